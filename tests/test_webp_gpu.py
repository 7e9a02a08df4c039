"""The lossless / animated WebP path on the GPU, stage by stage and whole, against tests/webp_model.py (integer numpy and plain
Python statements of the same rules) and against Pillow's libwebp decoder.  Everything is integer work, so the transform's
flags, modes and residual bytes, the coder's lengths and bytes, and the files are EQUAL to the model's; nothing is written
beyond a stream's length."""

import functools
import io
import warnings

import numpy as np
import pytest
import torch

from tests import webp_model as wm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (1, 16, 16), (3, 48, 80), (2, 50, 37), (1, 144, 256)]   # one pixel; small; odd sizes, a short last strip; many chunks
KINDS = ("noise", "scene", "correlated")
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    n, h, w = shape
    if kind == "correlated":
        f = np.stack([wm.correlated_frame(h, w, seed=5 + i) for i in range(n)])
    else:
        f = (wm.noise_frames if kind == "noise" else wm.scene_frames)(n, h, w, seed=sum(shape) + len(kind))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def transformed_of(shape, kind, pred_bits):
    """-> (flags (n,), modes (n, bh, bw), residual (n, h, w, 4)) of the model"""
    parts = [wm.transform(f, pred_bits) for f in frames_of(shape, kind)]
    out = (np.array([p[0] for p in parts], dtype=np.int32), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stream_of(shape, kind, i, pred_bits, group_bits):
    flags, modes, residual = transformed_of(shape, kind, pred_bits)
    return wm.encode_residual(shape[1], shape[2], int(flags[i]), modes[i], residual[i], pred_bits, group_bits)[0]


def decode(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(data)) as im:
            frames = []
            for i in range(getattr(im, "n_frames", 1)):
                im.seek(i)
                frames.append(np.asarray(im.convert("RGB")))
            return im.size, dict(im.info), frames


def test_pillow_decodes_webp():
    from PIL import features
    assert features.check("webp")


# ---------------------------------------------------------------------------------------------------- transform stage
def gpu_transform(frames, pred_bits):
    from vdpp_amd.hip import ops
    n, h, w, _ = frames.shape
    bs = 1 << pred_bits
    residual = torch.full((n, h, w, 4), FILL, dtype=torch.uint8, device=DEV)
    modes = torch.full((n, -(-h // bs), -(-w // bs)), FILL, dtype=torch.uint8, device=DEV)
    flags = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.webp_ws_bytes(n, h, w, pred_bits, 0), dtype=torch.uint8, device=DEV)
    ops.webp_transform(torch.from_numpy(np.array(frames)).to(DEV), residual, modes, flags, ws, pred_bits=pred_bits)
    torch.cuda.synchronize()
    return flags.cpu().numpy(), modes.cpu().numpy(), residual.cpu().numpy()


def check_transform(frames, pred_bits, what, want=None):
    if want is None:
        parts = [wm.transform(f, pred_bits) for f in frames]
        want = (np.array([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]))
    flags, modes, residual = gpu_transform(frames, pred_bits)
    bad = np.argwhere(flags != want[0])
    assert bad.size == 0, f"{what} pred_bits {pred_bits}: subtract-green flags differ first at frame {bad[0].tolist()}"
    bad = np.argwhere(modes != want[1])
    assert bad.size == 0, (f"{what} pred_bits {pred_bits}: modes differ first at (frame, block row, block) {bad[0].tolist()}: "
                           f"{modes[tuple(bad[0])]} for {want[1][tuple(bad[0])]}")
    bad = np.argwhere(residual != want[2])
    assert bad.size == 0, f"{what} pred_bits {pred_bits}: residual bytes differ first at (frame, y, x, byte) {bad[0].tolist()}"
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transform_stage_equals_the_model(shape):
    for kind in KINDS:
        for pred_bits in (2, 4):
            want = check_transform(frames_of(shape, kind), pred_bits, f"{shape} {kind}", transformed_of(shape, kind, pred_bits))
            if shape == (1, 144, 256) and kind != "noise":
                assert want[0].tolist() == [1 if kind == "correlated" else 0]


def test_transform_stage_picks_every_mode_and_takes_thin_and_ragged_frames():
    every = wm.every_mode_frame(2)
    _, modes, _ = wm.transform(every, 2)
    assert set(range(1, 14)) <= {int(m) for m in modes.reshape(-1)}, "every mode 1..13 must win some block of this frame"
    check_transform(every[None], 2, "every mode")
    check_transform(wm.noise_frames(2, 9, 1, 5), 2, "w = 1: no pixel to the left")
    check_transform(wm.scene_frames(2, 1, 33, 5), 3, "h = 1: no row above")
    check_transform(wm.scene_frames(1, 3, 5, 6), 3, "smaller than one block")
    check_transform(wm.scene_frames(1, 21, 300, 6), 3, "more columns than threads, ragged blocks")
    check_transform(wm.scene_frames(1, 13, 530, 7), 9, "a block wider than the workgroup")
    check_transform(wm.noise_frames(1, 40, 70, 7) // 64 * 64, 2, "many equal sums: the lowest mode among equals")


# ---------------------------------------------------------------------------------------------------- coder stage
def gpu_code(flags, modes, residual, pred_bits, group_bits):
    """-> (list of the frames' VP8L streams, the whole output buffer, lengths, cap)"""
    from vdpp_amd.hip import ops
    n, h, w, _ = residual.shape
    cap = ops.webp_stream_bytes(h, w, pred_bits, group_bits)
    out = torch.full((n, cap), FILL, dtype=torch.uint8, device=DEV)
    lens = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.webp_ws_bytes(n, h, w, pred_bits, group_bits), dtype=torch.uint8, device=DEV)
    ops.webp_code(torch.from_numpy(np.array(residual)).to(DEV), torch.from_numpy(np.array(modes)).to(DEV),
                  torch.from_numpy(np.array(flags, dtype=np.int32)).to(DEV), out, lens, ws, pred_bits=pred_bits, group_bits=group_bits)
    torch.cuda.synchronize()
    out, lens = out.cpu().numpy(), lens.cpu().numpy()
    return [out[i, :lens[i]].tobytes() for i in range(n)], out, lens, cap


def check_code(flags, modes, residual, pred_bits, group_bits, what, want=None):
    n, h, w, _ = residual.shape
    got, out, lens, cap = gpu_code(flags, modes, residual, pred_bits, group_bits)
    for i in range(n):
        ref = want[i] if want is not None else wm.encode_residual(h, w, int(flags[i]), modes[i], residual[i], pred_bits, group_bits)[0]
        assert 0 < lens[i] <= cap
        assert lens[i] == len(ref), f"{what} frame {i} group_bits {group_bits}: {lens[i]} bytes, the model has {len(ref)}"
        if got[i] != ref:
            at = next(k for k in range(len(ref)) if got[i][k] != ref[k])
            raise AssertionError(f"{what} frame {i} group_bits {group_bits}: first difference at byte {at} of {len(ref)}")
        assert np.all(out[i, lens[i]:] == FILL), f"{what} frame {i}: bytes beyond the stream were written"
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_coder_stage_is_byte_exact_on_the_models_residuals(shape):
    for kind in KINDS:
        flags, modes, residual = transformed_of(shape, kind, 3)
        for group_bits in (0, 2, 4):
            got = check_code(flags, modes, residual, 3, group_bits, f"{shape} {kind}",
                             want=[stream_of(shape, kind, i, 3, group_bits) for i in range(shape[0])])
            size, _, pictures = decode(wm.webp_file(got[0]))
            assert size == (shape[2], shape[1]) and np.array_equal(pictures[0], frames_of(shape, kind)[0])


def plain(residual_bgr):
    """(h, w, 3) B, G, R residuals -> the coder's inputs for one frame with mode 0 everywhere and no subtract green."""
    h, w, _ = residual_bgr.shape
    residual = np.zeros((1, h, w, 4), dtype=np.uint8)
    residual[0, :, :, :3] = residual_bgr
    return np.zeros(1, dtype=np.int32), np.zeros((1, -(-h // 4), -(-w // 4)), dtype=np.uint8), residual


def test_coder_stage_is_byte_exact_on_the_corners_of_the_coder():
    def record(inputs, group_bits):
        flags, modes, residual = inputs
        return wm.encode_residual(residual.shape[1], residual.shape[2], 0, modes[0], residual[0], 2, group_bits)[1]

    # a constant frame of literals only: every code is simple and the pixels take no bits
    const = plain(np.zeros((3, 1, 3), dtype=np.uint8))
    rec = record(const, 0)
    assert rec["strips"][0]["pixel_bits"] == 0 and all(c[2]["simple"] for c in rec["strips"][0]["codes"])
    check_code(*const, 2, 0, "three black pixels")
    # a constant frame: one literal and copies; with strips, runs that cross a strip's end and stop there
    const = plain(np.full((40, 50, 3), 0, dtype=np.uint8))
    for group_bits in (0, 2, 4):
        rec = record(const, group_bits)
        assert all(s["tokens"][0][0] == "lit" and all(k == "copy" for k, _ in s["tokens"][1:]) for s in rec["strips"])
        check_code(*const, 2, group_bits, "a constant frame")
    # alpha bytes of the residual are ignored
    dirty = (const[0], const[1], const[2].copy())
    dirty[2][..., 3] = 77
    assert check_code(*dirty, 2, 2, "alpha ignored", want=[wm.encode_residual(40, 50, 0, const[1][0], const[2][0], 2, 2)[0]])
    # a run of more than 4096 equal pixels, over several chunks: copies of 4096 and the remainders 0 .. 3 behind them
    for extra in (1, 2, 3, 4):
        total = 2 * 4096 + extra
        long_run = plain(np.full((1, total, 3), 9, dtype=np.uint8))
        rec = record(long_run, 0)
        rem = (total - 1) % 4096
        assert [v for k, v in rec["strips"][0]["tokens"] if k == "copy"] == [4096, 4096] + ([rem] if rem >= 3 else [])
        check_code(*long_run, 2, 0, f"a run of 2 * 4096 + {extra}")
    # a Huffman code deeper than 15 before the counts are halved (green follows a Fibonacci series, no two equal neighbours)
    fib = wm.fibonacci_values()
    assert fib.size == 11 * 995
    grid = np.zeros((11, 995, 3), dtype=np.uint8)
    grid[:, :, 1] = fib.reshape(11, 995)
    rec = record(plain(grid), 0)
    assert rec["strips"][0]["codes"][0][2]["halvings"] >= 1 and all(k == "lit" for k, _ in rec["strips"][0]["tokens"])
    check_code(*plain(grid), 2, 0, "Fibonacci counts")
    # an alphabet of two symbols
    two = np.zeros((8, 9, 3), dtype=np.uint8)
    two[:, :, 1] = (np.arange(72).reshape(8, 9) % 2) * 200
    rec = record(plain(two), 2)
    assert all(sorted(set(s["codes"][0][2]["lengths"])) == [0, 1] for s in rec["strips"])
    check_code(*plain(two), 2, 2, "two symbols")
    # runs of every short length, and runs that cross the ends of rows but not of strips
    rng = np.random.default_rng(8)
    runs = np.repeat(rng.integers(0, 4, (3000, 3)), rng.integers(1, 7, 3000), axis=0)[:20 * 400].astype(np.uint8)
    for group_bits in (0, 2, 3):
        check_code(*plain(runs.reshape(20, 400, 3)), 2, group_bits, "short runs")
    # more groups than one byte of green holds: the group's number goes on in red
    tall = plain(rng.integers(0, 3, (1030, 2, 3)).astype(np.uint8))
    got = check_code(*tall, 2, 2, "258 groups")
    assert np.array_equal(decode(wm.webp_file(got[0]))[2][0], wm.untransform(0, tall[1][0], tall[2][0], 2))


def test_coder_stage_carries_the_bit_offsets_past_256_segments():
    # 130 strips of 4 rows: 2 + 2 * 130 = 262 segments, so the scan over their bit counts takes a second round of 256, which
    # starts from the first's sum
    narrow = plain(np.random.default_rng(12).integers(0, 256, (520, 1, 3)).astype(np.uint8))
    rec = wm.encode_residual(520, 1, 0, narrow[1][0], narrow[2][0], 2, 2)[1]
    assert len(rec["strips"]) == 130
    check_code(*narrow, 2, 2, "262 segments")


def test_stream_bound_holds_and_is_what_the_header_derives():
    from vdpp_amd.hip import ops
    assert wm.GROUP_HEADER_MAX == 3983 + 2 * 3647 + 8 == 11285 and wm.SUB_HEADER_MAX == 3983 + 3647 + 4 + 11 + 4 == 7649
    for h, w, pb, gb in ((64, 40, 2, 0), (64, 40, 3, 2), (50, 37, 4, 4), (576, 1024, 3, 4), (16384, 1024, 9, 9), (1, 1, 2, 0)):
        assert ops.webp_stream_bytes(h, w, pb, gb) == wm.stream_bound(h, w, pb, gb)
    bs, groups, across = 8, 16, 10
    bits = 50 + 7649 + 30 * (64 // bs) * (40 // bs) + 3 + (4 + 7649 + 30 * groups * across) + groups * 11285 + 45 * 64 * 40
    assert ops.webp_stream_bytes(64, 40, 3, 2) == -(-bits // 8)
    for bad in ((0, 4, 3, 4), (4, 16385, 3, 4), (8192, 4096, 3, 4), (4, 4, 1, 4), (4, 4, 10, 4), (4, 4, 3, 1), (4, 4, 3, 10)):
        assert ops.webp_stream_bytes(*bad) == 0 and ops.webp_ws_bytes(1, *bad) == 0
    noise = np.random.default_rng(2).integers(0, 256, (64, 40, 3), dtype=np.uint8)
    for gb in (0, 2, 4):
        got = check_code(*plain(noise), 2, gb, "noise residuals")
        print(f"64x40 group_bits {gb}: noise takes {len(got[0])} bytes of {ops.webp_stream_bytes(64, 40, 2, gb)}")
        assert len(got[0]) <= ops.webp_stream_bytes(64, 40, 2, gb)


# ---------------------------------------------------------------------------------------------------- whole path
@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_encoder_files_are_webp_file_of_the_model_streams_and_decode(shape):
    from vdpp_amd.models.image_io import WEBP_GROUP_BITS, WEBP_PRED_BITS, WebpEncoder, webp_file
    n, h, w = shape
    for kind in KINDS:
        frames = frames_of(shape, kind)
        on_gpu = torch.from_numpy(np.array(frames)).to(DEV)
        for pred_bits, group_bits in ((WEBP_PRED_BITS, WEBP_GROUP_BITS), (3, 0)):
            enc = WebpEncoder(DEV, h, w, pred_bits=pred_bits, group_bits=group_bits)
            files = enc.encode(on_gpu)
            assert isinstance(files, list) and len(files) == n and all(isinstance(f, bytes) for f in files)
            assert files == enc.encode(on_gpu), "a second call on the kept buffers gives other bytes"
            streams = [stream_of(shape, kind, i, pred_bits, group_bits) for i in range(n)]
            for i in range(n):
                assert files[i] == webp_file(streams[i]) == wm.webp_file(streams[i])
                size, _, pictures = decode(files[i])
                assert size == (w, h) and len(pictures) == 1 and np.array_equal(pictures[0], frames[i])
            movie = enc.encode_animation(on_gpu, fps=5)
            assert movie == wm.webp_animation(streams, w, h, 5)
            size, info, pictures = decode(movie)
            assert size == (w, h) and len(pictures) == n and all(np.array_equal(p, f) for p, f in zip(pictures, frames))
            assert info.get("duration") == 200 and info.get("loop") == 0
    assert (WebpEncoder(DEV, h, w).pred_bits, WebpEncoder(DEV, h, w).group_bits) == (3, 4) == (WEBP_PRED_BITS, WEBP_GROUP_BITS)


def test_encoder_refuses_other_frames():
    from vdpp_amd.hip import ops
    from vdpp_amd.models.image_io import WebpEncoder
    enc = WebpEncoder(DEV, 16, 32)
    for bad in (torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 16, 32, 3), device=DEV),
                torch.zeros((0, 16, 32, 3), dtype=torch.uint8, device=DEV), torch.zeros((16, 32, 3), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            enc.encode(bad)
        with pytest.raises(ValueError):
            enc.encode_animation(bad)
    for kw in ({"pred_bits": 1}, {"pred_bits": 10}, {"pred_bits": 2.5}, {"group_bits": 1}, {"group_bits": 10}, {"group_bits": -1},
               {"group_bits": True}):
        with pytest.raises(ValueError):
            WebpEncoder(DEV, 16, 32, **kw)
    for h, w in ((16385, 4), (4, 16385), (8192, 4096), (0, 4)):
        with pytest.raises(ValueError):
            WebpEncoder(DEV, h, w)
    with pytest.raises(ValueError):
        enc.encode_animation(torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device=DEV), fps=0)
    residual = torch.zeros((1, 16, 32, 4), dtype=torch.uint8, device=DEV)
    modes = torch.zeros((1, 2, 4), dtype=torch.uint8, device=DEV)
    flags = torch.zeros((1,), dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.webp_ws_bytes(1, 16, 32, 3, 2), dtype=torch.uint8, device=DEV)
    lens = torch.zeros((1,), dtype=torch.int32, device=DEV)
    cap = ops.webp_stream_bytes(16, 32, 3, 2)
    with pytest.raises(Exception):                                     # a slot below the bound is refused on the host
        ops.webp_code(residual, modes, flags, torch.zeros((1, cap - 1), dtype=torch.uint8, device=DEV), lens, ws, pred_bits=3, group_bits=2)
    with pytest.raises(Exception):
        ops.webp_code(residual, modes, flags, torch.zeros((1, cap), dtype=torch.uint8, device=DEV), lens, ws[:-8], pred_bits=3, group_bits=2)
    with pytest.raises(Exception):
        ops.webp_code(residual, modes, flags, torch.zeros((1, 1 << 20), dtype=torch.uint8, device=DEV), lens, ws, pred_bits=3, group_bits=1)
    with pytest.raises(Exception):
        ops.webp_code(residual, modes[:, :1], flags, torch.zeros((1, cap), dtype=torch.uint8, device=DEV), lens, ws, pred_bits=3, group_bits=2)
    with pytest.raises(Exception):
        ops.webp_transform(torch.zeros((1, 16, 32, 3), device=DEV), residual, modes, flags, ws, pred_bits=3)
    with pytest.raises(Exception):
        ops.webp_transform(torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device=DEV), residual, modes, flags, ws, pred_bits=1)
    with pytest.raises(Exception):
        ops.webp_transform(torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device=DEV), residual[..., :3], modes, flags, ws, pred_bits=3)
    out = torch.full((1, cap), FILL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    assert int(lens[0]) == 0 and bool((out == FILL).all()), "a refused call must launch nothing"
    ops.webp_code(residual, modes, flags, out, lens, ws, pred_bits=3, group_bits=2)                    # and this is taken
    torch.cuda.synchronize()
    assert int(lens[0]) > 0


# ---------------------------------------------------------------------------------------------------- call sites
@pytest.fixture(scope="module")
def decoder():
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    vcfg = VAEDecoderConfig.tiny(64)
    return TemporalDecoderHIP(vcfg, random_state_dict(vcfg, seed=19), DEV)


def test_frame_emitter_webp_output_and_save_frames_from_the_device(decoder, tmp_path):
    from vdpp_amd.models.edge_stages import FrameEmitter, decode_latents_uint8
    from vdpp_amd.models.image_io import WebpEncoder, save_frames
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

    emitter, out, files = run(2, output="webp", gif_fps=5)
    assert emitter.output == "webp" and sorted(files) == [0, 1]
    enc = WebpEncoder(DEV, 64, 128)
    with torch.no_grad():
        u8 = [decode_latents_uint8(out[i].contiguous(), decoder, 3) for i in range(2)]
    for i in range(2):
        assert isinstance(files[i], list) and len(files[i]) == 1 and isinstance(files[i][0], bytes)
        assert files[i][0] == enc.encode_animation(u8[i][0], fps=5)
        size, info, pictures = decode(files[i][0])
        assert size == (128, 64) and len(pictures) == 3 and info.get("duration") == 200 and info.get("loop") == 0
        assert all(np.array_equal(p, u8[i][0][k].cpu().numpy()) for k, p in enumerate(pictures))
    emitter, out2, last = run(2, output="webp", keep="last")
    with torch.no_grad():
        assert sorted(last) == [1] and last[1][0] == enc.encode_animation(decode_latents_uint8(out2[1].contiguous(), decoder, 3)[0], fps=7)
    assert run(1, output="webp", keep="none")[2] == {}
    with pytest.raises(ValueError):
        FrameEmitter(decoder, emitter.stage, 3, output="webp", check_finite=True)
    with pytest.raises(ValueError):
        FrameEmitter(decoder, emitter.stage, 3, output="webp", gif_fps=0)

    # save_frames from the device: the same bytes, as one animated file and as a pattern of stills
    frames = u8[0][0]
    path = tmp_path / "v.webp"
    assert save_frames(frames, str(path), fps=5) == [str(path)]
    assert path.read_bytes() == files[0][0]
    kinds = [k for k, _ in wm.walk_webp(path.read_bytes())]
    assert kinds == [b"VP8X", b"ANIM"] + [b"ANMF"] * 3
    names = save_frames(frames, str(tmp_path / "f_%03d.webp"))
    assert names == [str(tmp_path / f"f_{k:03d}.webp") for k in range(3)]
    assert [open(name, "rb").read() for name in names] == enc.encode(frames)
    for k, name in enumerate(names):
        size, _, pictures = decode(open(name, "rb").read())
        assert size == (128, 64) and np.array_equal(pictures[0], frames[k].cpu().numpy())
    with pytest.raises(ValueError):
        save_frames(frames, str(tmp_path / "w.webp"), fps=0)
    with pytest.raises(ValueError):
        save_frames(frames.float(), str(tmp_path / "w.webp"))
    assert not (tmp_path / "w.webp").exists()


def test_generate_mode_writes_an_animated_webp_from_the_device(monkeypatch, tmp_path):
    from PIL import Image
    from vdpp_amd.models.image_io import WebpEncoder
    from vdpp_amd.modes import generate
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    src = tmp_path / "in.png"
    Image.fromarray(wm.scene_frames(1, 90, 200, 3)[0]).save(src)

    def run(out, tag):
        generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_{tag}", "--log-level", "WARNING",
                       "--random-init", "--tiny", "--input-image", str(src), "--height", "64", "--width", "128",
                       "--num-frames", "3", "--total-steps", "2", "--output", str(out)])
        assert not torch.distributed.is_initialized()

    run(tmp_path / "out.webp", "webp")
    run(tmp_path / "x.npy", "npy")
    a = np.load(tmp_path / "x.npy")
    data = (tmp_path / "out.webp").read_bytes()
    assert data == WebpEncoder(DEV, 64, 128).encode_animation(torch.from_numpy(a).to(DEV), fps=7)
    size, info, pictures = decode(data)
    assert size == (128, 64) and len(pictures) == 3 and info.get("duration") == 143 and info.get("loop") == 0
    assert int(pictures[0].max()) > int(pictures[0].min())
    assert all(np.array_equal(p, a[k]) for k, p in enumerate(pictures))
