"""The animated-GIF path on the GPU, stage by stage and whole, against tests/gif_model.py (integer numpy and plain Python
statements of the same rules) and against Pillow.

Quantiser: all integer arithmetic, so palettes and indices are EQUAL to the model's.  Picture quality: Pillow's own median cut
of the same frame without dithering, minus 0.05 dB (the model clears that by +0.57 to +4.7 dB on these kinds of frames; the
margin absorbs print rounding only).  LZW stage and whole path: byte for byte, lengths equal, nothing written beyond them."""

import functools
import io
import warnings

import numpy as np
import pytest
import torch

from tests import gif_model as gm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (1, 16, 16), (3, 48, 80), (2, 50, 37), (1, 144, 256)]   # one pixel; one bin plane or so; odd sizes; 36 k pixels
KINDS = ("noise", "scene")
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    f = (gm.noise_frames if kind == "noise" else gm.scene_frames)(*shape, seed=sum(shape) + len(kind))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """-> (palettes, indices, entries in use) of the model."""
    res = gm.quantise_frames(frames_of(shape, kind))
    for a in res[:2]:
        a.setflags(write=False)
    return res


def gpu_quantise(frames):
    from vdpp_amd.hip import ops
    n, h, w, _ = frames.shape
    palette = torch.full((n, 256, 3), FILL, dtype=torch.uint8, device=DEV)
    indices = torch.full((n, h, w), FILL, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.gif_ws_bytes(n, h, w, 16), dtype=torch.uint8, device=DEV)
    ops.gif_quantise(torch.from_numpy(np.array(frames)).to(DEV), palette, indices, ws)
    torch.cuda.synchronize()
    return palette.cpu().numpy(), indices.cpu().numpy()


def check_quantiser(frames, want, what):
    palettes, indices = gpu_quantise(frames)
    for i in range(frames.shape[0]):
        bad = np.nonzero((palettes[i] != want[0][i]).any(axis=1))[0]
        assert bad.size == 0, f"{what} frame {i}: palette entries {bad[:8].tolist()} differ ({want[2][i]} in use)"
        wrong = np.count_nonzero(indices[i] != want[1][i])
        assert wrong == 0, f"{what} frame {i}: {wrong} of {indices[i].size} indices differ"
    return palettes, indices


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantiser_equals_the_model(shape):
    Image = pytest.importorskip("PIL.Image")
    for kind in KINDS:
        frames, want = frames_of(shape, kind), reference(shape, kind)
        palettes, indices = check_quantiser(frames, want, f"{shape} {kind}")
        for i in range(shape[0]):
            if len(np.unique(frames[i].reshape(-1, 3), axis=0)) <= 256:
                continue
            theirs = np.asarray(Image.fromarray(frames[i]).quantize(256, method=0, dither=Image.Dither.NONE).convert("RGB"))
            ours, pillow = gm.psnr(palettes[i][indices[i]], frames[i]), gm.psnr(theirs, frames[i])
            print(f"{shape} {kind} frame {i}: {ours:.3f} dB, Pillow's median cut {pillow:.3f} dB, {want[2][i]} entries")
            assert ours >= pillow - 0.05


def test_quantiser_on_constant_few_colour_and_flat_frames():
    rng = np.random.default_rng(11)
    constant = np.full((20, 24, 3), (13, 200, 77), dtype=np.uint8)                          # one box
    bins = rng.choice(32768, 200, replace=False)                                            # 200 colours in distinct bins
    colours = np.stack([bins >> 10, (bins >> 5) & 31, bins & 31], axis=1) * 8 + rng.integers(0, 8, (200, 3))
    few = colours[rng.permutation(np.arange(20 * 24) % 200).reshape(20, 24)].astype(np.uint8)
    flat = gm.noise_frames(1, 20, 24, seed=4)[0].copy()                                     # one bin plane along R: G and B
    flat[..., 1] = 96 + flat[..., 1] % 8                                                    # have zero extent, and stay so
    flat[..., 2] = 40 + flat[..., 2] % 8
    frames = np.stack([constant, few, flat])
    want = gm.quantise_frames(frames)
    assert want[2][0] == 1 and want[2][1] == 200 and want[2][2] == 32
    palettes, indices = check_quantiser(frames, want, "constant / few colours / one bin plane")
    assert np.array_equal(palettes[1][indices[1]], few), "a frame of at most 256 colours in distinct bins must come back exactly"
    assert not palettes[0][1:].any() and not indices[0].any()


# ---------------------------------------------------------------------------------------------------- LZW stage
def gpu_lzw(indices, strip_rows):
    """-> (list of the frames' image data, the whole output buffer, lengths, cap)"""
    from vdpp_amd.hip import ops
    n, h, w = indices.shape
    cap = ops.gif_stream_bytes(h, w, strip_rows)
    out = torch.full((n, cap), FILL, dtype=torch.uint8, device=DEV)
    lens = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.gif_ws_bytes(n, h, w, strip_rows), dtype=torch.uint8, device=DEV)
    ops.gif_lzw(torch.from_numpy(np.array(indices)).to(DEV), out, lens, ws, strip_rows=strip_rows)
    torch.cuda.synchronize()
    out, lens = out.cpu().numpy(), lens.cpu().numpy()
    return [out[i, :lens[i]].tobytes() for i in range(n)], out, lens, cap


def check_lzw(indices, strip_rows, what):
    got, out, lens, cap = gpu_lzw(indices, strip_rows)
    for i in range(indices.shape[0]):
        want, _ = gm.lzw_image_data(indices[i], strip_rows)
        assert 0 < lens[i] <= cap
        assert lens[i] == len(want), f"{what} frame {i} strip rows {strip_rows}: {lens[i]} bytes, the model has {len(want)}"
        if got[i] != want:
            at = next(k for k in range(len(want)) if got[i][k] != want[k])
            raise AssertionError(f"{what} frame {i} strip rows {strip_rows}: first difference at byte {at} of {len(want)}")
        assert np.all(out[i, lens[i]:] == FILL), f"{what} frame {i}: bytes beyond the data were written"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lzw_stage_is_byte_exact_on_the_models_indices(shape):
    for kind in KINDS:
        indices = reference(shape, kind)[1]
        for strip_rows in sorted({1, 3, 16, shape[1]}):
            check_lzw(indices, strip_rows, f"{shape} {kind}")


def test_lzw_stage_is_byte_exact_on_the_corners_of_the_coder():
    check_lzw(np.array([[[7]]], dtype=np.uint8), 1, "one pixel")
    check_lzw(np.array([[[7]]], dtype=np.uint8), 16, "one pixel")
    constant = np.full((1, 40, 100), 3, dtype=np.uint8)                                     # the longest matches
    for strip_rows in (1, 16, 40):
        check_lzw(constant, strip_rows, "constant frame")
    noise = gm.noise_indices(64, 128, 21)[None]                                             # 8192 pixels in one strip:
    _, strips = gm.lzw_image_data(noise[0], 64)                                             # the table fills inside it
    assert len(strips) == 1 and strips[0]["codes"] > gm.TABLE_END - gm.FIRST_FREE
    check_lzw(noise, 64, "noise in one strip")
    check_lzw(noise, 5, "noise, 13 strips")
    for free in (512, gm.TABLE_END):                                                        # the width change and the full
        idx = gm.strip_ending_at(free)                                                      # table on a strip boundary
        _, strips = gm.lzw_image_data(idx, 1)
        assert strips[0]["free"] == free
        print(f"a strip of {idx.shape[1]} pixels ends with the next free code at {free}, {strips[0]['bits']} bits")
        check_lzw(idx[None], 1, f"strip ending at {free}, then CLEAR")
        check_lzw(idx[None, :1], 1, f"strip ending at {free}, then EOI")
    phases = gm.noise_indices(9, 37, 3, levels=6)[None]
    _, strips = gm.lzw_image_data(phases[0], 2)
    ends = [(s["start_bit"] + s["bits"]) % 8 for s in strips]
    assert ends[0] != ends[1] and len(set(ends)) >= 3, "consecutive strips must end on different bit phases"
    check_lzw(phases, 2, "strips on different bit phases")
    whole = gm.frame_with_whole_blocks()
    data, _ = gm.lzw_image_data(whole, 2)
    assert (len(data) - 2) % 256 == 0, "the data must be a whole number of 255-byte sub-blocks"
    check_lzw(whole[None], 2, "a whole number of sub-blocks")
    check_lzw(gm.noise_indices(1, 4200, 8)[None], 1, "one long row")
    check_lzw(gm.noise_indices(1, 4200, 8, levels=3)[None], 16, "one long row, three levels")


def test_lzw_stage_carries_the_bit_offsets_past_256_strips():
    # 300 strips of one pixel row: the scan over the strips' bit counts takes a second round of 256, which starts from the
    # first's sum
    indices = gm.noise_indices(300, 1, 17)[None]
    _, strips = gm.lzw_image_data(indices[0], 1)
    assert indices.shape == (1, 300, 1) and len(strips) == 300
    check_lzw(indices, 1, "300 strips")


def test_stream_bound_holds_and_is_what_the_header_derives():
    from vdpp_amd.hip import ops
    entries = gm.TABLE_END - gm.FIRST_FREE
    assert entries == 3838
    for h, w, rows in ((64, 128, 64), (64, 128, 5), (64, 128, 1), (1, 4200, 1), (50, 37, 3), (576, 1024, 16)):
        strips = -(-h // rows)
        nbytes = -(-(9 + 12 * h * w + 12 * (h * w // entries) + 12 * strips) // 8)
        assert ops.gif_stream_bytes(h, w, rows) == 1 + nbytes + -(-nbytes // 255) + 1
        if h * w <= 8192:
            data, recs = gm.lzw_image_data(gm.noise_indices(h, w, 21), rows)
            print(f"{h}x{w} rows {rows}: noise takes {len(data)} bytes of {ops.gif_stream_bytes(h, w, rows)}")
            assert len(data) <= ops.gif_stream_bytes(h, w, rows)
            assert all(r["bits"] <= 9 + 12 * r["codes"] + 12 * (r["codes"] // entries) + 12 for r in recs)


# ---------------------------------------------------------------------------------------------------- whole path
def decode(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(data)) as im:
            frames = []
            for i in range(im.n_frames):
                im.seek(i)
                frames.append(np.asarray(im.convert("RGB")))
            return im.size, dict(im.info), frames


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_encoder_file_is_write_gif_of_the_stages_and_decodes(shape):
    pytest.importorskip("PIL.Image")
    from vdpp_amd.models.image_io import GifEncoder, write_gif
    n, h, w = shape
    for kind in KINDS:
        frames = frames_of(shape, kind)
        on_gpu = torch.from_numpy(np.array(frames)).to(DEV)
        palettes, indices = gpu_quantise(frames)
        for strip_rows in (16, 3):
            enc = GifEncoder(DEV, h, w, strip_rows=strip_rows)
            data = enc.encode(on_gpu)
            assert isinstance(data, bytes) and data == enc.encode(on_gpu), "a second call on the kept buffers gives other bytes"
            assert data == write_gif(None, palettes, gpu_lzw(indices, strip_rows)[0], w, h, 7)
            assert data == gm.gif_file(palettes, [gm.lzw_image_data(i, strip_rows)[0] for i in indices], w, h, 7)
            size, info, pictures = decode(data)
            assert size == (w, h) and len(pictures) == n and info.get("loop") == 0 and info.get("duration") == 140
            for i in range(n):
                assert np.array_equal(pictures[i], palettes[i][indices[i]])
    assert GifEncoder(DEV, h, w).strip_rows == 8                       # the fastest measured within 2.5 % of one dictionary per frame


def test_encoder_refuses_other_frames():
    from vdpp_amd.models.image_io import GifEncoder
    enc = GifEncoder(DEV, 16, 32)
    for bad in (torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 16, 32, 3), device=DEV),
                torch.zeros((0, 16, 32, 3), dtype=torch.uint8, device=DEV), torch.zeros((16, 32, 3), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            enc.encode(bad)
    for kw in ({"strip_rows": 0}, {"strip_rows": -2}, {"strip_rows": 1.5}, {"fps": 0}):
        with pytest.raises(ValueError):
            GifEncoder(DEV, 16, 32, **kw)
    with pytest.raises(ValueError):
        GifEncoder(DEV, 4097, 4096)
    from vdpp_amd.hip import ops
    idx = torch.zeros((1, 16, 32), dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.gif_ws_bytes(1, 16, 32, 4), dtype=torch.uint8, device=DEV)
    lens = torch.zeros((1,), dtype=torch.int32, device=DEV)
    with pytest.raises(Exception):                                     # a slot below the bound is refused on the host
        ops.gif_lzw(idx, torch.zeros((1, ops.gif_stream_bytes(16, 32, 4) - 1), dtype=torch.uint8, device=DEV), lens, ws, strip_rows=4)
    with pytest.raises(Exception):
        ops.gif_lzw(idx, torch.zeros((1, ops.gif_stream_bytes(16, 32, 4)), dtype=torch.uint8, device=DEV), lens, ws[:-8], strip_rows=4)
    with pytest.raises(Exception):
        ops.gif_lzw(idx, torch.zeros((1, 4096), dtype=torch.uint8, device=DEV), lens, ws, strip_rows=0)


# ---------------------------------------------------------------------------------------------------- call sites
@pytest.fixture(scope="module")
def decoder():
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    vcfg = VAEDecoderConfig.tiny(64)
    return TemporalDecoderHIP(vcfg, random_state_dict(vcfg, seed=19), DEV)


def test_frame_emitter_gif_output_and_save_frames_from_the_device(decoder, tmp_path):
    from vdpp_amd.models.edge_stages import FrameEmitter, decode_latents_uint8
    from vdpp_amd.models.image_io import GifEncoder, save_frames
    from vdpp_amd.models.svd_unet import StableVideoUNet
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict
    from vdpp_amd.pipeline import LatentSpec, PipelineConfig, PipelineStage
    dev = torch.device(DEV)
    ucfg = UNetConfig.tiny(64)
    model = StableVideoUNet(unet=SVDUNetHIP(ucfg, random_state_dict(ucfg, seed=0, dtype=torch.float16), dev),
                            timesteps=StableVideoUNet._default_timestep_schedule(2))
    torch.manual_seed(42)
    model.set_dummy_conditioning(1, 3, 8, 16, dev)
    spec = LatentSpec(shape=torch.Size((1, 4, 3, 8, 16)), dtype=torch.float16, device=dev)

    def supplier(i):
        g = torch.Generator().manual_seed(1000 + i)
        return (torch.randn(spec.shape, generator=g) * model.init_noise_sigma).half().to(dev)

    def run(samples, **kw):
        stage = PipelineStage(model, PipelineConfig(total_steps=2, timesteps=[0, 1], world_size=1, rank=0, latent_spec=spec))
        emitter = FrameEmitter(decoder, stage, 3, **kw)
        with torch.no_grad():
            out = stage.run_many(samples, input_supplier=supplier)
            stage.drain()
            return emitter, out, emitter.finish(samples)

    emitter, out, files = run(3, output="gif", gif_fps=5)
    assert emitter.output == "gif" and sorted(files) == [0, 1, 2]
    enc = GifEncoder(DEV, 64, 128, fps=5)
    with torch.no_grad():
        u8 = [decode_latents_uint8(out[i].contiguous(), decoder, 3) for i in range(3)]
    for i in range(3):
        assert isinstance(files[i], list) and len(files[i]) == 1 and isinstance(files[i][0], bytes)
        assert files[i][0] == enc.encode(u8[i][0])
        size, info, pictures = decode(files[i][0])
        assert size == (128, 64) and len(pictures) == 3 and info.get("duration") == 200
    assert len({files[i][0] for i in range(3)}) == 3, "three samples, three different files"
    emitter, out2, last = run(2, output="gif", keep="last")
    with torch.no_grad():
        assert sorted(last) == [1] and last[1][0] == GifEncoder(DEV, 64, 128).encode(decode_latents_uint8(out2[1].contiguous(), decoder, 3)[0])
    assert run(1, output="gif", keep="none")[2] == {}
    with pytest.raises(ValueError):
        FrameEmitter(decoder, emitter.stage, 3, output="gif", check_finite=True)
    for fps in (0, -2, "7", None):
        with pytest.raises(ValueError):
            FrameEmitter(decoder, emitter.stage, 3, output="gif", gif_fps=fps)

    # save_frames from the device: the same bytes
    path = tmp_path / "v.gif"
    assert save_frames(u8[0][0], str(path), fps=5) == [str(path)]
    assert path.read_bytes() == files[0][0]
    walked = gm.walk_gif(path.read_bytes())
    assert walked["size"] == (128, 64) and walked["loop"] == 0 and [f["delay"] for f in walked["frames"]] == [20, 20, 20]
    with pytest.raises(ValueError):
        save_frames(u8[0][0], str(tmp_path / "w.gif"), fps=0)
    assert not (tmp_path / "w.gif").exists()

    # the other outputs are what they were
    with torch.no_grad():
        _, out, frames = run(1, output="uint8")
        assert torch.equal(frames[0], decoder.decode_latents_uint8(out[0].contiguous(), 3))
        _, out, frames = run(1)
        assert frames[0].dtype == torch.float32 and torch.equal(frames[0], decoder.decode_latents(out[0].contiguous(), 3))
        _, out, jpegs = run(1, output="jpeg")
        from vdpp_amd.models.image_io import JpegEncoder
        assert jpegs[0][0] == JpegEncoder(DEV, 64, 128).encode(decode_latents_uint8(out[0].contiguous(), decoder, 3)[0])


def test_generate_mode_writes_a_gif_from_the_device(monkeypatch, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.modes import generate
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    src = tmp_path / "in.png"
    Image.fromarray(gm.scene_frames(1, 90, 200, 3)[0]).save(src)
    generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_gif", "--log-level", "WARNING",
                   "--random-init", "--tiny", "--input-image", str(src), "--height", "64", "--width", "128",
                   "--num-frames", "3", "--total-steps", "2", "--output", str(tmp_path / "out.gif")])
    assert not torch.distributed.is_initialized()
    data = (tmp_path / "out.gif").read_bytes()
    size, info, pictures = decode(data)
    assert size == (128, 64) and len(pictures) == 3 and info.get("loop") == 0
    assert all(p.shape == (64, 128, 3) for p in pictures) and int(pictures[0].max()) > int(pictures[0].min())
    walked = gm.walk_gif(data)                                         # the device route's file: a local table per frame, no
    assert len(walked["frames"]) == 3 and all(f["palette"].shape == (256, 3) for f in walked["frames"])   # global one
