"""The frame interpolator on the GPU against tests/interp_model.py: vectors before and after the median and the frames,
byte for byte (integer arithmetic on both sides, a unique least key: there is nothing to tolerate), at the smallest shapes
where the indexing can go wrong; then the rounds, the reuse of scratch, a second stream, and the call sites.

  2 x 16 x 16, R = 1 and 24    every read clamps; the grid is 2 x 2
  3 x 40 x 72, R = 16          odd block counts, more than one pair
  2 x 64 x 96, R = 7           a range that is no multiple of 4 (rows of the staged region that are no whole dwords)
  5 x 24 x 200, R = 16         a wide, flat grid
Inputs: noise; a translated crop; a constant frame, where every cost ties and the penalty and the index decide."""

import functools

import numpy as np
import pytest
import torch

from tests import interp_model as im

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [((2, 16, 16), 1), ((2, 16, 16), 24), ((3, 40, 72), 16), ((2, 64, 96), 7), ((5, 24, 200), 16)]
KINDS = ("noise", "moved", "flat")
FILL = 0x5A


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind) -> np.ndarray:
    n, h, w = shape
    rng = np.random.default_rng(n * 1000 + h + w + len(kind))
    if kind == "noise":
        f = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    elif kind == "moved":
        f = im.moving_crop(im.smoothed_noise(rng, h + 64, w + 64), h, w, (1, -1), n)
    else:
        f = np.full((n, h, w, 3), 200, np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(shape, kind, R, lam=4):
    res = im.interpolate_round(frames_of(shape, kind), R, lam)
    for a in res:
        a.setflags(write=False)
    return res


def gpu_round(frames, R, lam, with_raw=True):
    from vdpp_amd.hip import ops
    n, h, w, _ = frames.shape
    dev = torch.from_numpy(np.array(frames)).to(DEV)
    shape = (n - 1, h // 8, w // 8, 2)
    vectors = torch.full(shape, FILL, dtype=torch.int16, device=DEV)
    raw = torch.full(shape, FILL, dtype=torch.int16, device=DEV) if with_raw else None
    out = torch.full((2 * n - 1, h, w, 3), FILL, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.interp_ws_bytes(n, h, w, R), dtype=torch.uint8, device=DEV)
    ops.interp_motion(dev, vectors, ws, search_range=R, penalty=lam, raw_vectors=raw)
    ops.interp_compensate(dev, vectors, out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), vectors.cpu().numpy(), None if raw is None else raw.cpu().numpy()


def check(got, want, what):
    out, vectors, raw = got
    if raw is not None:
        bad = np.argwhere((raw != want[2]).any(axis=-1))
        assert bad.size == 0, (f"{what}: {len(bad)} raw vectors differ, first at (pair, by, bx) = {bad[0].tolist()}: "
                               f"{raw[tuple(bad[0])].tolist()} for {want[2][tuple(bad[0])].tolist()}")
    bad = np.argwhere((vectors != want[1]).any(axis=-1))
    assert bad.size == 0, f"{what}: {len(bad)} vectors differ after the median, first at {bad[0].tolist()}"
    bad = np.argwhere(out != want[0])
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at (frame, y, x, c) = {bad[0].tolist()}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,R", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-R{r}" for s, r in CASES])
def test_vectors_and_frames_equal_the_model(shape, R, kind):
    check(gpu_round(frames_of(shape, kind), R, 4), reference(shape, kind, R), f"{shape} R={R} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lam", [0, 255])
def test_penalty_extremes(lam, kind):
    shape, R = (3, 40, 72), 16
    check(gpu_round(frames_of(shape, kind), R, lam), reference(shape, kind, R, lam), f"lam={lam} {kind}")


def test_raw_vectors_are_optional():
    shape, R = (3, 40, 72), 16
    check(gpu_round(frames_of(shape, "noise"), R, 4, with_raw=False), reference(shape, "noise", R), "no raw_vectors")


def test_refusals():
    from vdpp_amd.hip import ops
    assert ops.interp_ws_bytes(2, 16, 16, 1) > 0
    for args in ((1, 16, 16, 8), (2, 12, 16, 8), (2, 16, 20, 8), (2, 16, 16, 0), (2, 16, 16, 25), (2, 8, 16, 4)):
        assert ops.interp_ws_bytes(*args) == 0, args
    f = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=DEV)
    v = torch.zeros((1, 2, 2, 2), dtype=torch.int16, device=DEV)
    ws = torch.zeros(ops.interp_ws_bytes(2, 16, 16, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ops.HipKernelError, match="ws_bytes"):
        ops.interp_motion(f, v, ws[:-1], search_range=8, penalty=4)
    for kw in ({"search_range": 0, "penalty": 4}, {"search_range": 25, "penalty": 4}, {"search_range": 8, "penalty": 256},
               {"search_range": 8, "penalty": -1}):
        with pytest.raises(ops.HipKernelError):
            ops.interp_motion(f, v, ws, **kw)
    with pytest.raises(ops.HipKernelError, match="multiples of 8"):
        ops.interp_motion(torch.zeros((2, 12, 16, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 1, 2, 2), dtype=torch.int16, device=DEV),
                          ws, search_range=8, penalty=4)
    with pytest.raises(ValueError):
        ops.interp_motion(f, v[:, :1], ws, search_range=8, penalty=4)
    with pytest.raises(ValueError):
        ops.interp_compensate(f, v, torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.interp_compensate(f.cpu(), v, torch.zeros((3, 16, 16, 3), dtype=torch.uint8, device=DEV))


# ---------------------------------------------------------------------------------------------------- FrameInterpolator
def test_factor_4_is_two_rounds_and_factor_1_is_the_input():
    from vdpp_amd.models.image_io import FrameInterpolator
    shape, R = (3, 40, 72), 16
    frames = frames_of(shape, "moved")
    dev = torch.from_numpy(np.array(frames)).to(DEV)
    assert FrameInterpolator(DEV, 40, 72, factor=1)(dev) is dev
    two = FrameInterpolator(DEV, 40, 72, factor=2, search_range=R)
    got = two(dev)
    assert got.shape == (5, 40, 72, 3) and got.dtype == torch.uint8 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), reference(shape, "moved", R)[0])
    assert np.array_equal(two.vectors.cpu().numpy(), reference(shape, "moved", R)[1])
    four = FrameInterpolator(DEV, 40, 72, factor=4, search_range=R)
    got = four(dev).cpu().numpy()
    want, want_vectors, _ = im.interpolate_round(reference(shape, "moved", R)[0], R, 4)
    assert got.shape == (9, 40, 72, 3) and np.array_equal(got, want)
    assert np.array_equal(got, im.interpolate(frames, 4, R, 4))
    assert np.array_equal(four.vectors.cpu().numpy(), want_vectors), "vectors are the last round's"
    for kw in ({"factor": 3}, {"factor": 0}, {"search_range": 0}, {"search_range": 25}, {"penalty": 256}, {"penalty": -1},
               {"search_range": 8.0}):
        with pytest.raises(ValueError):
            FrameInterpolator(DEV, 40, 72, **kw)
    for h, w in ((36, 72), (40, 70), (8, 72)):
        with pytest.raises(ValueError, match="multiples of 8"):
            FrameInterpolator(DEV, h, w)
    with pytest.raises(ValueError):
        two(dev[:, :32])


def test_reused_scratch_and_a_second_stream():
    from vdpp_amd.models.image_io import FrameInterpolator
    shape, R = (5, 24, 200), 16
    interp = FrameInterpolator(DEV, 24, 200, factor=2, search_range=R)
    noise = torch.from_numpy(np.array(frames_of(shape, "noise"))).to(DEV)
    moved = torch.from_numpy(np.array(frames_of(shape, "moved"))).to(DEV)
    first = interp(noise).cpu().numpy()
    buffers = {k: v.data_ptr() for k, v in interp._scratch.items()}
    assert np.array_equal(first, reference(shape, "noise", R)[0])
    assert np.array_equal(interp(moved).cpu().numpy(), reference(shape, "moved", R)[0])      # other frames through the same scratch
    assert np.array_equal(interp(noise).cpu().numpy(), first)
    assert {k: v.data_ptr() for k, v in interp._scratch.items()} == buffers, "scratch is kept per frame count"
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = interp(noise)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), first)


# ---------------------------------------------------------------------------------------------------- call sites
def test_save_frames_apng_from_the_device(tmp_path):
    from PIL import Image
    from vdpp_amd.models.image_io import save_frames
    shape, R = (3, 40, 72), 16
    dev = torch.from_numpy(np.array(frames_of(shape, "moved"))).to(DEV)
    path = tmp_path / "x.apng"
    assert save_frames(dev, str(path), fps=5, interpolate=2) == [str(path)]
    want = reference(shape, "moved", R)[0]
    with Image.open(path) as img:
        assert img.n_frames == 5
        for i in range(5):
            img.seek(i)
            assert np.array_equal(np.asarray(img.convert("RGB")), want[i]), f"frame {i}"
            assert img.info["duration"] == 100.0, "5 fps doubled: 100 ms per frame"
    with pytest.raises(ValueError, match="multiples of 8"):
        save_frames(dev[:, :36], str(tmp_path / "y.apng"), fps=5, interpolate=2)
    with pytest.raises(ValueError, match="device"):
        save_frames(dev.cpu(), str(tmp_path / "y.apng"), fps=5, interpolate=2)
    assert not (tmp_path / "y.apng").exists()
    plain = tmp_path / "p.apng"
    save_frames(dev, str(plain), fps=5)
    one = tmp_path / "q.apng"
    save_frames(dev, str(one), fps=5, interpolate=1)
    assert one.read_bytes() == plain.read_bytes()


def test_save_frames_refuses_the_target_before_it_interpolates(monkeypatch, tmp_path):
    from vdpp_amd.models import image_io

    def ran(*args, **kw):
        raise AssertionError("the search ran for frames that cannot be written")

    monkeypatch.setattr(image_io.ops, "interp_motion", ran)
    dev = torch.from_numpy(np.array(frames_of((3, 40, 72), "moved"))).to(DEV)
    for name, kw, message in (("x.mp4", {}, "ffmpeg"), ("x.xyz", {}, "unknown output format"), ("x.png", {}, "pattern"),
                              ("x.jpg", {}, "pattern"), ("x.avi", {"quality": 0}, "quality"), ("x.avi", {"fps": 2.5}, "fps"),
                              ("x.avi", {"fps": 0}, "fps"), ("x.gif", {"fps": 0}, "fps"), ("x.apng", {"fps": -1}, "fps"),
                              ("x.webp", {"fps": "7"}, "fps"), ("x.apng", {"interp_range": 25}, "search_range"),
                              ("x.apng", {"interp_penalty": True}, "penalty")):
        with pytest.raises(ValueError, match=message):
            image_io.save_frames(dev, str(tmp_path / name), interpolate=2, **kw)
    assert list(tmp_path.iterdir()) == []


def emitter_rig(videos):
    """The tiny random-init model with ``videos`` videos per sample: ``(decoder, run)``, where ``run(samples, **kw)`` pipelines
    that many samples into a ``FrameEmitter(**kw)`` and returns it with what it kept."""
    from vdpp_amd.models.edge_stages import FrameEmitter
    from vdpp_amd.models.svd_unet import StableVideoUNet
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig
    from vdpp_amd.models.vae_hip import random_state_dict as vae_state_dict
    from vdpp_amd.pipeline import LatentSpec, PipelineConfig, PipelineStage
    dev = torch.device(DEV)
    vcfg = VAEDecoderConfig.tiny(64)
    decoder = TemporalDecoderHIP(vcfg, vae_state_dict(vcfg, seed=19), DEV)
    ucfg = UNetConfig.tiny(64)
    model = StableVideoUNet(unet=SVDUNetHIP(ucfg, random_state_dict(ucfg, seed=0, dtype=torch.float16), dev),
                            timesteps=StableVideoUNet._default_timestep_schedule(2))
    torch.manual_seed(42)
    model.set_dummy_conditioning(videos, 3, 8, 16, dev)
    spec = LatentSpec(shape=torch.Size((videos, 4, 3, 8, 16)), dtype=torch.float16, device=dev)

    def supplier(i):
        g = torch.Generator().manual_seed(1000 + i)
        return (torch.randn(spec.shape, generator=g) * model.init_noise_sigma).half().to(dev)

    def run(samples, **kw):
        stage = PipelineStage(model, PipelineConfig(total_steps=2, timesteps=[0, 1], world_size=1, rank=0, latent_spec=spec))
        emitter = FrameEmitter(decoder, stage, 3, **kw)
        with torch.no_grad():
            stage.run_many(samples, input_supplier=supplier)
            stage.drain()
            return emitter, emitter.finish(samples)

    return decoder, run


def test_frame_emitter_interpolates_uint8_output():
    from vdpp_amd.models.edge_stages import FrameEmitter
    decoder, run = emitter_rig(1)
    _, plain = run(2, output="uint8", interpolate=1)
    emitter, doubled = run(2, output="uint8", interpolate=2, interp_range=8)
    assert sorted(plain) == sorted(doubled) == [0, 1]
    for i in range(2):
        assert plain[i].shape == (1, 3, 64, 128, 3) and doubled[i].shape == (1, 5, 64, 128, 3)
        want = im.interpolate(plain[i][0].cpu().numpy(), 2, 8, 4)
        assert np.array_equal(doubled[i][0].cpu().numpy(), want), f"sample {i}"
    # an animated output plays the longer video at the doubled rate: 5 frames of 100 ms for 3 frames at 5 fps
    import io
    from PIL import Image
    _, gifs = run(1, output="gif", gif_fps=5, interpolate=2, interp_range=8)
    with Image.open(io.BytesIO(gifs[0][0])) as img:
        assert img.n_frames == 5 and img.size == (128, 64) and img.info.get("duration") == 100
    with pytest.raises(ValueError, match="interpolate"):
        FrameEmitter(decoder, emitter.stage, 3, output="float32", interpolate=2)
    for kw in ({"interpolate": 3}, {"interpolate": 2, "interp_range": 0}, {"interpolate": 4, "interp_penalty": 256},
               {"interpolate": 2, "interp_range": True}, {"interpolate": 2, "interp_penalty": 4.0}):
        with pytest.raises(ValueError):
            FrameEmitter(decoder, emitter.stage, 3, output="uint8", **kw)
    # the interpolator's own check: integers of numpy pass as they do there
    taken = FrameEmitter(decoder, emitter.stage, 3, output="uint8", interpolate=2, interp_range=np.int64(8), interp_penalty=np.uint8(0))
    assert (taken.interp_range, taken.interp_penalty) == (8, 0)


def test_frame_emitter_interpolates_each_video_of_a_sample():
    """Two distinct videos in one sample (the benchmark's micro-batch): the interpolator's buffers are reused from video to
    video, and each video must still come out as its own interpolation, in the kept frames and in what an encoder sees."""
    from vdpp_amd.models.image_io import GifEncoder
    _, run = emitter_rig(2)
    _, plain = run(1, output="uint8", interpolate=1)
    _, doubled = run(1, output="uint8", interpolate=2, interp_range=8)
    assert plain[0].shape == (2, 3, 64, 128, 3) and doubled[0].shape == (2, 5, 64, 128, 3)
    videos = plain[0].cpu().numpy()
    assert not np.array_equal(videos[0], videos[1]), "the test needs two different videos"
    for v in range(2):
        assert np.array_equal(doubled[0][v].cpu().numpy(), im.interpolate(videos[v], 2, 8, 4)), f"video {v}"
    _, gifs = run(1, output="gif", gif_fps=5, interpolate=2, interp_range=8)
    encoder = GifEncoder(DEV, 64, 128, fps=10)
    for v in range(2):
        assert gifs[0][v] == encoder.encode(doubled[0][v]), f"video {v}: the GIF of its own interpolated frames"


def test_generate_mode_interpolates_before_it_writes(monkeypatch, tmp_path, caplog):
    from PIL import Image
    from vdpp_amd.modes import generate
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    src = tmp_path / "in.png"
    Image.fromarray(im.smoothed_noise(np.random.default_rng(4), 90, 200)).save(src)

    def run(out, tag, *extra):
        generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_{tag}", "--log-level", "INFO",
                       "--random-init", "--tiny", "--input-image", str(src), "--height", "64", "--width", "128",
                       "--num-frames", "3", "--total-steps", "2", "--output", str(out), *extra])
        assert not torch.distributed.is_initialized()

    run(tmp_path / "plain.npy", "plain")
    with caplog.at_level("INFO"):
        run(tmp_path / "four.npy", "four", "--interpolate", "4", "--interp-range", "8", "--interp-penalty", "2")
    plain, four = np.load(tmp_path / "plain.npy"), np.load(tmp_path / "four.npy")
    assert plain.shape == (3, 64, 128, 3) and four.shape == (9, 64, 128, 3)
    assert np.array_equal(four, im.interpolate(plain, 4, 8, 2))
    assert any("interpolated 3 frames at 7 fps to 9 at 28 fps" in r.getMessage() for r in caplog.records)
    # (--fps is also part of the model's conditioning, so it stays what it was: the file plays at 2 x 7)
    run(tmp_path / "two.apng", "two", "--interpolate", "2", "--interp-range", "8", "--interp-penalty", "2")
    with Image.open(tmp_path / "two.apng") as img:
        assert img.n_frames == 5 and img.info["duration"] == pytest.approx(1000.0 / 14)
        img.seek(1)
        assert np.array_equal(np.asarray(img.convert("RGB")), four[2])
