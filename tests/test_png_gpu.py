"""The PNG / APNG path on the GPU, stage by stage and whole, against tests/png_model.py (integer numpy and plain Python
statements of the same rules) and against Pillow.  Everything is integer work, so the filter's tags and bytes, the deflate
stage's lengths and bytes, and the files are EQUAL to the model's; nothing is written beyond a stream's length."""

import functools
import io
import warnings
import zlib

import numpy as np
import pytest
import torch

from tests import png_model as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (1, 16, 16), (3, 48, 80), (2, 50, 37), (1, 144, 256)]   # one pixel; small; odd sizes; strips of many chunks
KINDS = ("noise", "scene")
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    f = (pm.noise_frames if kind == "noise" else pm.scene_frames)(*shape, seed=sum(shape) + len(kind))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def filtered_of(shape, kind):
    f = pm.filter_frames(frames_of(shape, kind))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def stream_of(shape, kind, i, strip_rows):
    return pm.deflate_stream(filtered_of(shape, kind)[i], strip_rows)[0]


# ---------------------------------------------------------------------------------------------------- filter stage
def gpu_filter(frames):
    from vdpp_amd.hip import ops
    n, h, w, _ = frames.shape
    out = torch.full((n, h, 1 + 3 * w), FILL, dtype=torch.uint8, device=DEV)
    ops.png_filter(torch.from_numpy(np.array(frames)).to(DEV), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_filter(frames, what):
    got, want = gpu_filter(frames), pm.filter_frames(frames)
    bad = np.argwhere(got[:, :, 0] != want[:, :, 0])
    assert bad.size == 0, f"{what}: filter types differ first at (frame, row) {bad[0].tolist()}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: filtered bytes differ first at {bad[0].tolist()}"
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_filter_stage_equals_the_model(shape):
    for kind in KINDS:
        got = gpu_filter(frames_of(shape, kind))
        want = filtered_of(shape, kind)
        assert np.array_equal(got[:, :, 0], want[:, :, 0]), f"{shape} {kind}: filter types differ"
        assert np.array_equal(got, want), f"{shape} {kind}: filtered bytes differ first at {np.argwhere(got != want)[0].tolist()}"


def test_filter_stage_picks_every_kind_of_filter_and_takes_thin_frames():
    ramps = pm.ramps()
    want = pm.filter_frames(ramps)
    assert len({int(t) for t in want[:, :, 0].reshape(-1)}) >= 4, "the ramps and the noise must pick at least four filter types"
    check_filter(ramps, "ramps")
    check_filter(pm.noise_frames(2, 9, 1, 5), "w = 1: no pixel to the left")
    check_filter(pm.scene_frames(2, 1, 33, 5), "h = 1: no row above")
    assert (1 + 3 * 22) % 2 == 1
    check_filter(pm.scene_frames(1, 7, 22, 6), "an odd pitch")
    check_filter(pm.scene_frames(1, 3, 300, 6), "more bytes than threads in a row")


# ---------------------------------------------------------------------------------------------------- deflate stage
def gpu_deflate(filtered, strip_rows):
    """-> (list of the frames' zlib streams, the whole output buffer, lengths, cap)"""
    from vdpp_amd.hip import ops
    n, h, pitch = filtered.shape
    w = (pitch - 1) // 3
    cap = ops.png_stream_bytes(h, w, strip_rows)
    out = torch.full((n, cap), FILL, dtype=torch.uint8, device=DEV)
    lens = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.png_ws_bytes(n, h, w, strip_rows), dtype=torch.uint8, device=DEV)
    ops.png_deflate(torch.from_numpy(np.array(filtered)).to(DEV), out, lens, ws, strip_rows=strip_rows)
    torch.cuda.synchronize()
    out, lens = out.cpu().numpy(), lens.cpu().numpy()
    return [out[i, :lens[i]].tobytes() for i in range(n)], out, lens, cap


def check_deflate(filtered, strip_rows, what, want=None):
    got, out, lens, cap = gpu_deflate(filtered, strip_rows)
    for i in range(filtered.shape[0]):
        ref = want[i] if want is not None else pm.deflate_stream(filtered[i], strip_rows)[0]
        assert 0 < lens[i] <= cap
        assert lens[i] == len(ref), f"{what} frame {i} strip rows {strip_rows}: {lens[i]} bytes, the model has {len(ref)}"
        if got[i] != ref:
            at = next(k for k in range(len(ref)) if got[i][k] != ref[k])
            raise AssertionError(f"{what} frame {i} strip rows {strip_rows}: first difference at byte {at} of {len(ref)}")
        assert np.all(out[i, lens[i]:] == FILL), f"{what} frame {i}: bytes beyond the stream were written"
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_deflate_stage_is_byte_exact_on_the_models_filtered_bytes(shape):
    for kind in KINDS:
        filtered = filtered_of(shape, kind)
        for strip_rows in sorted({1, 3, 16, shape[1]}):
            got = check_deflate(filtered, strip_rows, f"{shape} {kind}",
                                want=[stream_of(shape, kind, i, strip_rows) for i in range(shape[0])])
            assert zlib.decompress(got[0]) == filtered[0].tobytes()


def rows_of(data, pitch):
    """Bytes -> (1, h, pitch): the deflate stage takes any bytes as rows."""
    a = np.asarray(data, dtype=np.uint8)
    assert a.size % pitch == 0 and (pitch - 1) % 3 == 0
    return a.reshape(1, -1, pitch)


def test_deflate_stage_is_byte_exact_on_the_corners_of_the_coder():
    # constant strips whose one run has 258 k + {1, 2, 3, 4} bytes: remainders 0 .. 3 behind the leading literal
    for k, extra in ((1, 1), (2, 2), (3, 3), (1, 4)):
        total = 258 * k + extra
        pitch = next(p for p in range(4, total + 1, 3) if total % p == 0)      # (a pitch is 1 + 3w)
        const = rows_of(np.full(total, 9), pitch)
        rows = const.shape[1]
        _, strips = pm.deflate_stream(const[0], rows)
        rem = (total - 1) % 258
        assert len(strips) == 1 and strips[0]["matches"] == [258] * k + ([rem] if rem >= 3 else [])
        assert len(strips[0]["tokens"]) == 1 + k + (1 if rem >= 3 else rem) and strips[0]["literals"] == [9], "one literal value"
        check_deflate(const, rows, f"a run of 258 * {k} + {extra}")
    # more than a chunk of equal bytes, and matches that start near a chunk's end
    check_deflate(rows_of(np.full(3 * 4099, 7), 4099), 3, "a run over three chunks")
    check_deflate(rows_of(np.full(3 * 4099, 7), 4099), 1, "a run per strip")
    # a Huffman code deeper than 15 before the counts are halved
    fib = pm.fibonacci_row()
    _, strips = pm.deflate_stream(fib[None], 1)
    assert fib.size == 1 + 3 * 1400 and strips[0]["halvings"] >= 1 and not strips[0]["matches"]          # and no match at all
    check_deflate(fib[None, None], 1, "Fibonacci counts")
    # a strip that is a single match behind its literal
    single = rows_of(np.full(4, 0), 4)
    _, strips = pm.deflate_stream(single[0], 1)
    assert strips[0]["tokens"] == [("lit", 0), ("match", 3)]
    check_deflate(single, 1, "literal and one match")
    # consecutive strips that end on different bit phases
    phases = pm.filter_frames(pm.noise_frames(1, 9, 5, 3) // 40)
    _, strips = pm.deflate_stream(phases[0], 2)
    ends = [(s["start_bit"] + s["bits"]) % 8 for s in strips]
    assert len(set(ends)) >= 3, f"the strips must end on at least three bit phases: {ends}"
    check_deflate(phases, 2, "strips on different bit phases")
    # runs of every short length, and runs that cross the ends of rows but not of strips
    rng = np.random.default_rng(8)
    runs = np.repeat(rng.integers(0, 4, 3000), rng.integers(1, 7, 3000))[:8 * 1000].astype(np.uint8)
    for strip_rows in (1, 3, 8):
        check_deflate(rows_of(runs, 1000), strip_rows, "short runs")
    long_runs = np.repeat(rng.integers(0, 256, 40), rng.integers(200, 900, 40))[:16 * 700].astype(np.uint8)
    for strip_rows in (1, 5, 16):
        check_deflate(rows_of(long_runs, 700), strip_rows, "long runs")


def test_deflate_stage_carries_the_bit_offsets_past_256_strips():
    # 300 strips of one row: the scan over the strips' bit counts takes a second round of 256, which starts from the first's sum
    filtered = pm.filter_frames(pm.noise_frames(1, 300, 1, 11))
    assert filtered.shape == (1, 300, 4)
    want, strips = pm.deflate_stream(filtered[0], 1)
    ends = {(s["start_bit"] + s["bits"]) % 8 for s in strips}
    assert len(strips) == 300 and len(ends) >= 3, f"300 strips that end on mixed bit phases: {len(strips)}, {sorted(ends)}"
    assert zlib.decompress(want) == filtered[0].tobytes()
    check_deflate(filtered, 1, "300 strips", want=[want])


def test_stream_bound_holds_and_is_what_the_header_derives():
    from vdpp_amd.hip import ops
    assert pm.HEADER_BITS_MAX == 3 + 14 + 19 * 3 + 288 * 14 == 4106
    for h, w, rows in ((64, 128, 64), (64, 128, 5), (64, 128, 1), (1, 1400, 1), (50, 37, 3), (576, 1024, 8)):
        strips = -(-h // rows)
        bits = strips * (4106 + 15) + 15 * h * (1 + 3 * w)
        assert ops.png_stream_bytes(h, w, rows) == 2 + -(-bits // 8) + 4
    noise = np.random.default_rng(2).integers(0, 256, (1, 64, 1 + 3 * 40), dtype=np.uint8)
    for rows in (1, 5, 64):
        got = check_deflate(noise, rows, "noise")
        print(f"64x40 rows {rows}: noise takes {len(got[0])} bytes of {ops.png_stream_bytes(64, 40, rows)}")
        assert len(got[0]) <= ops.png_stream_bytes(64, 40, rows)


# ---------------------------------------------------------------------------------------------------- whole path
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


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_encoder_files_are_png_file_of_the_stages_and_decode(shape):
    pytest.importorskip("PIL.Image")
    from vdpp_amd.models.image_io import PngEncoder, png_file
    n, h, w = shape
    for kind in KINDS:
        frames = frames_of(shape, kind)
        on_gpu = torch.from_numpy(np.array(frames)).to(DEV)
        filtered = gpu_filter(frames)
        for strip_rows in (16, 3):
            enc = PngEncoder(DEV, h, w, strip_rows=strip_rows)
            files = enc.encode(on_gpu)
            assert isinstance(files, list) and len(files) == n and all(isinstance(f, bytes) for f in files)
            assert files == enc.encode(on_gpu), "a second call on the kept buffers gives other bytes"
            streams = gpu_deflate(filtered, strip_rows)[0]
            for i in range(n):
                assert files[i] == png_file(h, w, streams[i])
                assert files[i] == pm.png_file(h, w, stream_of(shape, kind, i, strip_rows))
                size, _, pictures = decode(files[i])
                assert size == (w, h) and len(pictures) == 1 and np.array_equal(pictures[0], frames[i])
            size, info, pictures = decode(enc.encode_apng(on_gpu, fps=5))
            assert size == (w, h) and len(pictures) == n and all(np.array_equal(p, f) for p, f in zip(pictures, frames))
            assert abs(info.get("duration") - 200.0) < 1e-6
    assert PngEncoder(DEV, h, w).strip_rows == 16         # profiles/png_timing.txt: the fastest of 4 / 8 / 16 / 32 rows within 1 %


def test_encoder_refuses_other_frames():
    from vdpp_amd.hip import ops
    from vdpp_amd.models.image_io import PngEncoder
    enc = PngEncoder(DEV, 16, 32)
    for bad in (torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 16, 32, 3), device=DEV),
                torch.zeros((0, 16, 32, 3), dtype=torch.uint8, device=DEV), torch.zeros((16, 32, 3), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            enc.encode(bad)
    for kw in ({"strip_rows": 0}, {"strip_rows": -2}, {"strip_rows": 1.5}):
        with pytest.raises(ValueError):
            PngEncoder(DEV, 16, 32, **kw)
    with pytest.raises(ValueError):
        PngEncoder(DEV, 4097, 4096)
    filtered = torch.zeros((1, 16, 97), dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.png_ws_bytes(1, 16, 32, 4), dtype=torch.uint8, device=DEV)
    lens = torch.zeros((1,), dtype=torch.int32, device=DEV)
    cap = ops.png_stream_bytes(16, 32, 4)
    with pytest.raises(Exception):                                     # a slot below the bound is refused on the host
        ops.png_deflate(filtered, torch.zeros((1, cap - 1), dtype=torch.uint8, device=DEV), lens, ws, strip_rows=4)
    with pytest.raises(Exception):
        ops.png_deflate(filtered, torch.zeros((1, cap), dtype=torch.uint8, device=DEV), lens, ws[:-8], strip_rows=4)
    with pytest.raises(Exception):
        ops.png_deflate(filtered, torch.zeros((1, 65536), dtype=torch.uint8, device=DEV), lens, ws, strip_rows=0)
    with pytest.raises(Exception):
        ops.png_filter(torch.zeros((1, 16, 32, 3), device=DEV), filtered)
    with pytest.raises(Exception):
        ops.png_filter(torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device=DEV), filtered[:, :, :96])
    ops.png_deflate(filtered, torch.zeros((1, cap), dtype=torch.uint8, device=DEV), lens, ws, strip_rows=4)   # and this is taken
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- call sites
@pytest.fixture(scope="module")
def decoder():
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    vcfg = VAEDecoderConfig.tiny(64)
    return TemporalDecoderHIP(vcfg, random_state_dict(vcfg, seed=19), DEV)


def test_frame_emitter_png_output_and_save_frames_from_the_device(decoder, tmp_path):
    from vdpp_amd.models.edge_stages import FrameEmitter, decode_latents_uint8
    from vdpp_amd.models.image_io import PngEncoder, save_frames
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

    emitter, out, files = run(2, output="png")
    assert emitter.output == "png" and sorted(files) == [0, 1]
    enc = PngEncoder(DEV, 64, 128)
    with torch.no_grad():
        u8 = [decode_latents_uint8(out[i].contiguous(), decoder, 3) for i in range(2)]
    for i in range(2):
        assert isinstance(files[i], list) and len(files[i]) == 1 and len(files[i][0]) == 3
        assert files[i][0] == enc.encode(u8[i][0])
        for k in range(3):
            size, _, pictures = decode(files[i][0][k])
            assert size == (128, 64) and np.array_equal(pictures[0], u8[i][0][k].cpu().numpy())
    emitter, out2, last = run(2, output="png", keep="last")
    with torch.no_grad():
        assert sorted(last) == [1] and last[1][0] == enc.encode(decode_latents_uint8(out2[1].contiguous(), decoder, 3)[0])
    assert run(1, output="png", keep="none")[2] == {}
    with pytest.raises(ValueError):
        FrameEmitter(decoder, emitter.stage, 3, output="png", check_finite=True)

    # save_frames from the device: the same bytes, as a directory, a pattern and one animated file
    want = files[0][0]
    names = save_frames(u8[0][0], str(tmp_path / "dir"))
    assert names == [str(tmp_path / "dir" / f"{k:03d}.png") for k in range(3)]
    assert [open(name, "rb").read() for name in names] == want
    names = save_frames(u8[0][0], str(tmp_path / "f_%03d.png"))
    assert names == [str(tmp_path / f"f_{k:03d}.png") for k in range(3)] and [open(name, "rb").read() for name in names] == want
    path = tmp_path / "v.apng"
    assert save_frames(u8[0][0], str(path), fps=5) == [str(path)]
    assert path.read_bytes() == enc.encode_apng(u8[0][0], fps=5)
    idats = [p for k, p in pm.walk_png(path.read_bytes()) if k in (b"IDAT", b"fdAT")]
    assert [idats[0]] + [p[4:] for p in idats[1:]] == [p for f in want for k, p in pm.walk_png(f) if k == b"IDAT"]
    size, info, pictures = decode(path.read_bytes())
    assert size == (128, 64) and len(pictures) == 3 and all(np.array_equal(p, u8[0][0][k].cpu().numpy()) for k, p in enumerate(pictures))
    with pytest.raises(ValueError):
        save_frames(u8[0][0], str(tmp_path / "x.png"))
    with pytest.raises(ValueError):
        save_frames(u8[0][0], str(tmp_path / "w.apng"), fps=0)
    assert not (tmp_path / "x.png").exists() and not (tmp_path / "w.apng").exists()


def test_generate_mode_writes_png_frames_from_the_device(monkeypatch, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.models.image_io import PngEncoder
    from vdpp_amd.modes import generate
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    src = tmp_path / "in.png"
    Image.fromarray(pm.scene_frames(1, 90, 200, 3)[0]).save(src)

    def run(out, tag):
        generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_{tag}", "--log-level", "WARNING",
                       "--random-init", "--tiny", "--input-image", str(src), "--height", "64", "--width", "128",
                       "--num-frames", "3", "--total-steps", "2", "--output", str(out)])
        assert not torch.distributed.is_initialized()

    run(tmp_path / "frames", "png")
    run(tmp_path / "x.npy", "npy")
    a = np.load(tmp_path / "x.npy")
    want = PngEncoder(DEV, 64, 128).encode(torch.from_numpy(a).to(DEV))
    names = sorted(p.name for p in (tmp_path / "frames").iterdir())
    assert names == ["000.png", "001.png", "002.png"]
    for k, name in enumerate(names):
        data = (tmp_path / "frames" / name).read_bytes()
        assert data == want[k], f"{name} is not the encoder's file of the .npy frames"
        size, _, pictures = decode(data)
        assert size == (128, 64) and pictures[0].shape == (64, 128, 3) and int(pictures[0].max()) > int(pictures[0].min())
        assert np.array_equal(pictures[0], a[k])
