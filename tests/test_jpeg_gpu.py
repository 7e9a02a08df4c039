"""The JPEG frame encoder on the GPU, stage by stage and whole, against tests/jpeg_model.py (an fp64 / integer statement
of the same specification and a bit-level Huffman writer in plain Python) and against Pillow.

Coefficient stage: a coefficient may differ from the fp64 statement by one, and only where the fp64 value before rounding
lies within BAND = 2e-3 (unquantised units) of a rounding boundary: twice the worst case of an fp32 8 + 8-term DCT on
|x| <= 128 (16 roundings x 2^-24 x 1024 ~ 1e-3).  At least 98 % of every case's coefficients must lie outside that band,
so the band cannot swallow the comparison.  Entropy stage and whole path: byte for byte.  Picture quality: Pillow's own
encode of the same picture at the same quality, minus 0.05 dB."""

import functools
import io
import warnings

import numpy as np
import pytest
import torch

from tests import jpeg_model as jm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND, OUTSIDE_BAND = 2e-3, 0.98
SHAPES = [(1, 16, 16), (3, 48, 80), (2, 50, 37), (1, 32, 1040)]        # one MCU; 15 MCUs; edges replicated; 65 MCUs per row
KINDS = ("noise", "scene")
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    """Seeded frames.  A case of a few hundred coefficients can hold more than 2 % exact ties by chance (at quality 100 the
    (0,0), (0,4), (4,0) and (4,4) terms are multiples of 1/8), so, by the fp64 statement alone, the seed moves on until
    98.5 % of the coefficients lie outside the band at quality 100, the quality with the most ties."""
    for seed in range(sum(shape) + len(kind), 10 ** 6):
        f = (jm.noise_frames if kind == "noise" else jm.scene_frames)(*shape, seed=seed)
        _, unquantised, div = jm.coefficients(f, 100)
        if 1.0 - jm.near_boundary(unquantised, div, BAND).mean() >= 0.985:
            f.setflags(write=False)
            return f


@functools.lru_cache(maxsize=None)
def reference(shape, kind, quality):
    return jm.coefficients(frames_of(shape, kind), quality)


def gpu_coefficients(frames, quality):
    from vdpp_amd.hip import ops
    n, h, w, _ = frames.shape
    coef = torch.full((n, *ops.jpeg_mcu_grid(h, w), 6, 64), 0x7777, dtype=torch.int16, device=DEV)
    ops.jpeg_dct_quant(torch.from_numpy(np.array(frames)).to(DEV), coef, quality=quality)
    return coef


def check_coefficients(got, want, f, div, what):
    diff = got.astype(np.int64) - want.astype(np.int64)
    band = jm.near_boundary(f, div, BAND)
    outside = 1.0 - band.mean()
    print(f"{what}: {np.count_nonzero(diff)} of {diff.size} coefficients differ, largest {np.abs(diff).max()}, "
          f"{outside:.3%} lie outside the band")
    assert np.abs(diff).max() <= 1, f"{what}: a coefficient is {np.abs(diff).max()} off"
    assert not np.any((diff != 0) & ~band), f"{what}: {np.count_nonzero((diff != 0) & ~band)} coefficients differ outside the band"
    assert outside >= OUTSIDE_BAND, f"{what}: only {outside:.2%} of the coefficients lie outside the band"


@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_coefficients_match_the_fp64_statement(shape, quality):
    for kind in KINDS:
        want, f, div = reference(shape, kind, quality)
        got = gpu_coefficients(frames_of(shape, kind), quality).cpu().numpy()
        assert got.shape == want.shape
        check_coefficients(got, want, f, div, f"{shape} {kind} q{quality}")


def test_coefficients_of_extreme_blocks_at_quality_100():
    """Blocks of 0 / 255 in the sign patterns of the bases (0,4), (4,0) and (4,4), grey so that Y is the pattern itself: the
    largest AC magnitudes 8-bit samples give (every |c(4, x)| is sqrt(1/8), so the sums are 32 * 255 / 8 = 1020: the
    +-1023 clamp of the kernel is a guard these blocks stay under, not a value they reach)."""
    d = jm.dct_matrix()
    frame = np.zeros((1, 16, 48, 3), dtype=np.uint8)
    for m, (u, v) in enumerate(((0, 4), (4, 0), (4, 4))):
        pattern = np.where(np.outer(d[u], d[v]) > 0, 255, 0).astype(np.uint8)
        if m == 2:
            pattern = 255 - pattern                                    # the other sign: -128 where the basis is positive
        frame[0, :, 16 * m:16 * m + 16] = np.tile(pattern, (2, 2))[:, :, None]
    want, f, div = jm.coefficients(frame, 100)
    got = gpu_coefficients(frame, 100).cpu().numpy()
    peak = np.abs(f[0, 0, :, :4]).max(axis=(1, 2))
    print("largest |coefficient| per MCU before rounding:", peak, "quantised:", np.abs(want[0, 0, :, :4]).max(axis=(1, 2)))
    assert np.all(peak >= 1019.9) and np.abs(want[..., 1:]).max() <= 1023
    diff = got.astype(np.int64) - want
    assert np.abs(diff).max() <= 1 and not np.any((diff != 0) & ~jm.near_boundary(f, div, BAND))
    assert np.array_equal(np.abs(got[0, 0, :, :4]).max(axis=(1, 2)), np.abs(want[0, 0, :, :4]).max(axis=(1, 2)))


# ---------------------------------------------------------------------------------------------------- entropy stage
def gpu_entropy(coef, restart):
    """-> (list of the frames' segments, the whole output buffer, lengths, cap)"""
    from vdpp_amd.hip import ops
    n, rows, cols = coef.shape[:3]
    cap = ops.jpeg_stream_bytes(rows * 16, cols * 16, restart)
    out = torch.full((n, cap), FILL, dtype=torch.uint8, device=DEV)
    lens = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.jpeg_entropy_ws_bytes(n, rows, cols, restart), dtype=torch.uint8, device=DEV)
    ops.jpeg_entropy(torch.from_numpy(np.ascontiguousarray(coef)).to(DEV), out, lens, ws, restart_mcus=restart)
    torch.cuda.synchronize()
    out, lens = out.cpu().numpy(), lens.cpu().numpy()
    return [out[i, :lens[i]].tobytes() for i in range(n)], out, lens, cap


def check_entropy(coef, restart, what):
    got, out, lens, cap = gpu_entropy(coef, restart)
    for i in range(coef.shape[0]):
        want, _ = jm.entropy_segment(coef[i], restart)
        assert 0 < lens[i] <= cap
        assert lens[i] == len(want), f"{what} frame {i} restart {restart}: {lens[i]} bytes, the writer has {len(want)}"
        if got[i] != want:
            at = next(k for k in range(len(want)) if got[i][k] != want[k])
            raise AssertionError(f"{what} frame {i} restart {restart}: first difference at byte {at} of {len(want)}")
        assert np.all(out[i, lens[i]:] == FILL), f"{what} frame {i}: bytes beyond the segment were written"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entropy_stage_is_bit_exact_on_picture_coefficients(shape):
    cols = -(-shape[2] // 16)
    restarts = (1, 3, 5) if shape == (3, 48, 80) else sorted({1, cols, 2 * cols + 1})
    for kind, quality in (("scene", 90), ("noise", 100), ("scene", 50)):
        coef = reference(shape, kind, quality)[0]
        for restart in restarts:
            check_entropy(coef, restart, f"{shape} {kind} q{quality}")


def corner_frame(rng):
    """(2, 6, 6, 64): the corners of the coder, block by block; what is left over is sparse random data."""
    c = np.zeros((12, 6, 64), dtype=np.int16)
    k = 0

    def block():
        nonlocal k
        b = c[k // 6, k % 6]
        k += 1
        return b

    block()                                                            # all zero (and the first block of the frame)
    block()[63] = 1                                                    # a lone last coefficient: ZRLs, no EOB
    block()[63] = -1023
    for run in (15, 16, 31, 47):                                       # zero runs around the ZRL boundary, then EOB
        block()[1 + run] = 1
        b = block(); b[1] = -1; b[2 + run] = 1023
    b = block(); b[1:64] = 1                                           # no zero at all
    b = block(); b[1:64] = -1
    b = block(); b[1:64:2] = 1023; b[2:64:2] = -1023
    b = block(); b[16] = 1; b[33] = -1; b[50] = 5; b[63] = 7           # runs of 15, 16, 16 and 12 to the end
    b = block(); b[48] = -300; b[49] = 300                             # a run of 47, then none
    while k < 72:
        b = block()
        idx = rng.choice(np.arange(1, 64), size=rng.integers(0, 8), replace=False)
        b[idx] = rng.integers(-1023, 1024, size=len(idx))
    # DC: steps of +-2047 between neighbours of every component (category 11), first differences of +-1023 / -1024
    dc = np.where(np.arange(12 * 4) % 2 == 0, 1023, -1024).reshape(12, 4)
    c[:, :4, 0] = dc
    c[:, 4, 0] = np.where(np.arange(12) % 2 == 0, -1024, 1023)
    c[:, 5, 0] = np.where(np.arange(12) % 2 == 0, 1023, -1024)
    c[5, :, 0] = 0                                                     # and differences of zero further on
    c[6, :, 0] = 0
    c[6, 0] = 0                                                        # an all-zero block after a zero DC: 2 + 4 bits
    c[6, 4] = 0
    return c.reshape(2, 6, 6, 64)


def dense_frame(restarts):
    """Dense large values, reseeded until the reference stream of every restart in `restarts` holds a stuffed FF 00 and
    at least one interval that needs no padding."""
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        c = rng.integers(-1023, 1024, size=(2, 6, 6, 64)).astype(np.int16)
        good = True
        for restart in restarts:
            data, pads = jm.entropy_segment(c, restart)
            good = good and b"\xff\x00" in data and 0 in pads
        if good:
            return c, seed
    raise AssertionError("no seed gives a stuffed byte and an unpadded interval")


def test_entropy_stage_is_bit_exact_on_the_corners_of_the_coder():
    restarts = (1, 5, 12)
    dense, seed = dense_frame(restarts)
    worst = np.full((2, 6, 6, 64), 1023, dtype=np.int16)               # every block at 20 + 63 * 26 bits but for the DC runs
    worst[..., 1::2] = -1023
    worst[..., 0] = np.where(np.arange(6) % 2 == 0, 1023, -1024)
    coef = np.stack([corner_frame(np.random.default_rng(7)), dense, worst])
    for restart in restarts:
        data, pads = jm.entropy_segment(coef[1], restart)
        assert b"\xff\x00" in data and 0 in pads, "the dense frame must hold a stuffed byte and an unpadded interval"
        print(f"dense frame (seed {seed}), restart {restart}: {data.count(bytes([255, 0]))} stuffed bytes, padding {pads}")
        check_entropy(coef, restart, "corner / dense / longest-code frames")
    # the bound behind every buffer, from the tables themselves: no block of either kind passes 20 + 63 * 26 bits.  A symbol
    # (run, size) fills run + 1 coefficient slots with its code and `size` further bits
    for dc, ac in ((0, 2), (1, 3)):
        dc_bits = max(length + sym for sym, (_, length) in jm.CODES[dc].items())
        slot_bits = max((length + (sym & 15)) / ((sym >> 4) + 1) for sym, (_, length) in jm.CODES[ac].items())
        print(f"tables {dc}/{ac}: a DC term takes at most {dc_bits} bits, an AC slot at most {slot_bits}")
        assert dc_bits + 63 * slot_bits <= 20 + 63 * 26
    assert jm.CODES[2][0x0A][1] + 10 == 26 and jm.CODES[0][11][1] + 11 == 20       # the luminance block reaches the bound


def test_entropy_stage_carries_the_offsets_past_256_intervals():
    # one MCU row of 300 MCUs, an interval each: the scan over the intervals' lengths takes a second round of 256, which starts
    # from the first's sum; RSTm runs through 0 .. 7 many times
    coef = jm.coefficients(jm.scene_frames(1, 16, 4800, seed=31), 90)[0]
    assert coef.shape[:3] == (1, 1, 300)
    want, _ = jm.entropy_segment(coef[0], 1)
    assert [want.count(bytes([0xFF, 0xD0 + m])) >= 37 for m in range(8)] == [True] * 8
    check_entropy(coef, 1, "300 intervals")


# ---------------------------------------------------------------------------------------------------- whole path
def pillow_jpeg(frame, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def decode(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            return im.size, np.asarray(im.convert("RGB"))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_encoder_files_are_header_scan_eoi_and_decode_like_pillows(shape):
    pytest.importorskip("PIL.Image")
    from vdpp_amd.models.image_io import JpegEncoder, jpeg_header
    n, h, w = shape
    cols = -(-w // 16)
    for kind in KINDS:
        frames = frames_of(shape, kind)
        on_gpu = torch.from_numpy(np.array(frames)).to(DEV)
        for quality, restart in ((90, None), (50, 1)) + (((90, 3), (100, 5)) if shape == (3, 48, 80) else ()):
            enc = JpegEncoder(DEV, h, w, quality=quality, restart_mcus=restart)
            assert enc.restart_mcus == (restart or cols)
            files = enc.encode(on_gpu)
            assert files == enc.encode(on_gpu), "a second call on the kept buffers gives other bytes"
            coef = gpu_coefficients(frames, quality).cpu().numpy()
            assert len(files) == n
            for i, data in enumerate(files):
                want = jpeg_header(h, w, quality, enc.restart_mcus) + jm.entropy_segment(coef[i], enc.restart_mcus)[0] + b"\xff\xd9"
                assert data == want
                size, got = decode(data)
                assert size == (w, h)
                ours, theirs = jm.psnr(got, frames[i]), jm.psnr(decode(pillow_jpeg(frames[i], quality))[1], frames[i])
                print(f"{shape} {kind} q{quality} restart {enc.restart_mcus} frame {i}: {ours:.3f} dB, Pillow {theirs:.3f} dB, "
                      f"{len(data)} bytes, Pillow {len(pillow_jpeg(frames[i], quality))}")
                assert ours >= theirs - 0.05


def test_encoder_refuses_other_frames():
    from vdpp_amd.models.image_io import JpegEncoder
    enc = JpegEncoder(DEV, 16, 32)
    for bad in (torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 16, 32, 3), device=DEV),
                torch.zeros((0, 16, 32, 3), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            enc.encode(bad)
    with pytest.raises(ValueError):
        JpegEncoder(DEV, 16, 32, quality=0)
    with pytest.raises(ValueError):
        JpegEncoder(DEV, 16, 32, restart_mcus=65536)


# ---------------------------------------------------------------------------------------------------- call sites
@pytest.fixture(scope="module")
def decoder():
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    vcfg = VAEDecoderConfig.tiny(64)
    return TemporalDecoderHIP(vcfg, random_state_dict(vcfg, seed=19), DEV)


def test_frame_emitter_jpeg_output_and_save_frames_from_the_device(decoder, tmp_path):
    from vdpp_amd.models.edge_stages import FrameEmitter, decode_latents_uint8
    from vdpp_amd.models.image_io import JpegEncoder, save_frames
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

    emitter, out, files = run(3, output="jpeg", jpeg_quality=80)
    assert emitter.output == "jpeg" and sorted(files) == [0, 1, 2]
    enc = JpegEncoder(DEV, 64, 128, quality=80)
    with torch.no_grad():
        u8 = [decode_latents_uint8(out[i].contiguous(), decoder, 3) for i in range(3)]
    for i in range(3):
        assert isinstance(files[i], list) and len(files[i]) == 1 and all(isinstance(b, bytes) for b in files[i][0])
        assert files[i][0] == enc.encode(u8[i][0])
        assert decode(files[i][0][0])[0] == (128, 64)
    assert len({files[i][0][0] for i in range(3)}) == 3, "three samples, three different first frames"
    emitter, out2, last = run(2, output="jpeg", keep="last")
    with torch.no_grad():
        assert sorted(last) == [1] and last[1][0] == JpegEncoder(DEV, 64, 128).encode(decode_latents_uint8(out2[1].contiguous(), decoder, 3)[0])
    assert run(1, output="jpeg", keep="none")[2] == {}
    with pytest.raises(ValueError):
        FrameEmitter(decoder, emitter.stage, 3, output="jpeg", check_finite=True)
    with pytest.raises(ValueError):
        FrameEmitter(decoder, emitter.stage, 3, output="jpeg", jpeg_quality=0)

    # save_frames from the device: the same bytes, in the container and as single files
    path = tmp_path / "v.avi"
    assert save_frames(u8[0][0], str(path), fps=6, quality=80) == [str(path)]
    res = jm.walk_avi(path.read_bytes())
    assert res["frames"] == files[0][0]
    assert [size for _, _, _, size in res["index"]] == [len(f) for f in files[0][0]]
    assert res["avih"][4] == 3 and res["avih"][8:10] == (128, 64) and res["avih"][0] == 1000000 // 6
    names = save_frames(u8[0][0], str(tmp_path / "f_%03d.jpg"), quality=80)
    assert [open(n, "rb").read() for n in names] == files[0][0]

    # the other two outputs are what they were
    with torch.no_grad():
        _, out, frames = run(1, output="uint8")
        assert torch.equal(frames[0], decoder.decode_latents_uint8(out[0].contiguous(), 3))
        _, out, frames = run(1)
        assert frames[0].dtype == torch.float32 and torch.equal(frames[0], decoder.decode_latents(out[0].contiguous(), 3))


def test_generate_mode_writes_a_video_file(monkeypatch, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.modes import generate
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    src = tmp_path / "in.png"
    Image.fromarray(jm.scene_frames(1, 90, 200, 3)[0]).save(src)

    def run(out, tag, *more):
        generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_{tag}", "--log-level", "WARNING",
                       "--random-init", "--tiny", "--input-image", str(src), "--height", "64", "--width", "128",
                       "--num-frames", "3", "--total-steps", "2", "--output", str(out), *more])
        assert not torch.distributed.is_initialized()

    run(tmp_path / "out.avi", "avi")
    res = jm.walk_avi((tmp_path / "out.avi").read_bytes())
    assert res["avih"][4] == 3 and res["avih"][8:10] == (128, 64) and len(res["index"]) == 3
    pictures = [decode(f) for f in res["frames"]]
    assert all(size == (128, 64) for size, _ in pictures)
    run(tmp_path / "f_%03d.jpg", "jpg", "--jpeg-quality", "60")
    small = [open(tmp_path / f"f_{i:03d}.jpg", "rb").read() for i in range(3)]
    for data, (_, at90) in zip(small, pictures):
        size, at60 = decode(data)
        assert size == (128, 64) and jm.psnr(at60, at90) > 25          # the same frames, at another quality
    assert sum(map(len, small)) < sum(map(len, res["frames"]))
