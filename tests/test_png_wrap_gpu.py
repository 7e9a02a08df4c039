"""PNG and APNG files put together on the GPU (sp_png_wrap: chunks, their CRC-32, an animation's frames at the exclusive sum of
their lengths) against the host's statement of the same files, image_io.png_file / write_apng, and against tests/png_model.py
and Pillow.  The streams are those of the deflate stage, which tests/test_png_gpu.py holds to the model; everything is integer
work, so the files are EQUAL, and nothing is written beyond a file's length."""

import functools
import io
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import png_model as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (3, 48, 80), (2, 50, 37), (1, 144, 256)]     # one frame (no fdAT) and several; odd sizes; a long stream
KINDS = ("noise", "scene")
FPS = (5, 7, 12.5)
FILL = 0xA5
STRIP_ROWS = 16


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    f = (pm.noise_frames if kind == "noise" else pm.scene_frames)(*shape, seed=sum(shape) + len(kind))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def streams_of(shape, kind):
    """-> (the frames' zlib streams on the device (n, cap), their lengths there, the streams as bytes): made once per case."""
    from vdpp_amd.models.image_io import PngEncoder
    enc = PngEncoder(DEV, shape[1], shape[2], strip_rows=STRIP_ROWS, assemble="host")
    out, lens = enc.enqueue(torch.from_numpy(np.array(frames_of(shape, kind))).to(DEV))
    torch.cuda.synchronize()
    return out.clone(), lens.clone(), tuple(enc.collect_streams(out, lens))


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


def wrap(shape, kind, animate, delay=(1, 7), file_cap=None, ws_short=0):
    """-> (files buffer as numpy, file_len as numpy)"""
    from vdpp_amd.hip import ops
    n, h, w = shape
    out, lens, _ = streams_of(shape, kind)
    if file_cap is None:
        file_cap = ops.apng_file_bytes(n, h, w, STRIP_ROWS) if animate else ops.png_file_bytes(h, w, STRIP_ROWS)
    files = torch.full((file_cap,) if animate else (n, file_cap), FILL, dtype=torch.uint8, device=DEV)
    file_len = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.png_wrap_ws_bytes(n, out.shape[1]) - ws_short, dtype=torch.uint8, device=DEV)
    ops.png_wrap(out, lens, files, file_len, ws, height=h, width=w, animate=animate, delay=delay)
    torch.cuda.synchronize()
    return files.cpu().numpy(), file_len.cpu().numpy()


def first_difference(got, want):
    return next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stills_equal_png_file_and_nothing_beyond_them_is_written(shape, kind):
    pytest.importorskip("PIL.Image")
    from vdpp_amd.models.image_io import png_file
    n, h, w = shape
    streams = streams_of(shape, kind)[2]
    files, file_len = wrap(shape, kind, False)
    for i in range(n):
        want = png_file(h, w, streams[i])
        assert want == pm.png_file(h, w, streams[i])
        assert file_len[i] == len(streams[i]) + 57 == len(want)
        got = files[i, :file_len[i]].tobytes()
        assert got == want, f"{shape} {kind} frame {i}: first difference at byte {first_difference(got, want)} of {len(want)}"
        assert np.all(files[i, file_len[i]:] == FILL), f"{shape} {kind} frame {i}: bytes beyond the file were written"
        assert [k for k, _ in pm.walk_png(got)] == [b"IHDR", b"IDAT", b"IEND"]
        size, _, pictures = decode(got)                      # (Pillow checks every chunk's CRC)
        assert size == (w, h) and len(pictures) == 1 and np.array_equal(pictures[0], frames_of(shape, kind)[i])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_animation_equals_write_apng_and_nothing_beyond_it_is_written(shape, kind):
    pytest.importorskip("PIL.Image")
    from vdpp_amd.models.image_io import write_apng
    n, h, w = shape
    streams = list(streams_of(shape, kind)[2])
    for fps in FPS:
        delay = (1 / Fraction(fps)).limit_denominator(65535)
        data, file_len = wrap(shape, kind, True, delay=(delay.numerator, delay.denominator))
        want = write_apng(None, streams, w, h, fps)
        assert want == pm.apng_file(streams, w, h, fps)
        assert file_len[0] == len(want) and np.all(file_len[1:] == -1), "file_len[0] is the length, the other words stay"
        got = data[:file_len[0]].tobytes()
        assert got == want, f"{shape} {kind} fps {fps}: first difference at byte {first_difference(got, want)} of {len(want)}"
        assert np.all(data[file_len[0]:] == FILL), f"{shape} {kind} fps {fps}: bytes beyond the file were written"
    kinds = [k for k, _ in pm.walk_png(got)]
    assert kinds == [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n - 1) + [b"IEND"]
    size, info, pictures = decode(got)
    assert size == (w, h) and len(pictures) == n and all(np.array_equal(p, f) for p, f in zip(pictures, frames_of(shape, kind)))
    if n > 1:
        assert abs(info.get("duration") - 1000.0 / FPS[-1]) < 1e-6


def test_more_frames_than_threads_follow_one_another():
    # 260 frames of one pixel: the scan over the chunk sizes takes a second round of 256, which starts from the first's sum,
    # and the stills' loop a second turn
    from vdpp_amd.models.image_io import png_file, write_apng
    shape, kind = (260, 1, 1), "noise"
    streams = list(streams_of(shape, kind)[2])
    data, file_len = wrap(shape, kind, True)
    want = write_apng(None, streams, 1, 1, 7)
    assert want == pm.apng_file(streams, 1, 1, 7)
    assert file_len[0] == len(want) and np.all(file_len[1:] == -1)
    got = data[:file_len[0]].tobytes()
    assert got == want, f"260 frames: first difference at byte {first_difference(got, want)} of {len(want)}"
    assert np.all(data[file_len[0]:] == FILL), "260 frames: bytes beyond the file were written"
    files, file_len = wrap(shape, kind, False)
    for i in range(260):
        want = png_file(1, 1, streams[i])
        got = files[i, :file_len[i]].tobytes()
        assert got == want, f"still {i} of 260: first difference at byte {first_difference(got, want)} of {len(want)}"
        assert np.all(files[i, file_len[i]:] == FILL), f"still {i} of 260: bytes beyond the file were written"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_encoder_routes_give_the_same_bytes_call_after_call(shape):
    from vdpp_amd.models.image_io import PNG_ASSEMBLE, PngEncoder
    n, h, w = shape
    for kind in KINDS:
        x = torch.from_numpy(np.array(frames_of(shape, kind))).to(DEV)
        dev, host = PngEncoder(DEV, h, w, assemble="device"), PngEncoder(DEV, h, w, assemble="host")
        files = dev.encode(x)
        assert isinstance(files, list) and len(files) == n and all(isinstance(f, bytes) for f in files)
        assert files == host.encode(x)
        assert files == dev.encode(x), "a second call on the kept buffers gives other bytes"
        for fps in (5, 12.5):
            movie = dev.encode_apng(x, fps=fps)
            assert isinstance(movie, bytes) and movie == host.encode_apng(x, fps=fps)
            assert movie == dev.encode_apng(x, fps=fps), "a second call on the kept buffers gives other bytes"
        assert files == dev.encode(x), "the animation's buffers are not the stills'"
    assert PngEncoder(DEV, h, w).assemble == PNG_ASSEMBLE


def test_refusals():
    from vdpp_amd.hip import ops
    from vdpp_amd.models.image_io import PngEncoder
    shape = (3, 48, 80)
    n, h, w = shape
    cap = streams_of(shape, "scene")[0].shape[1]
    assert ops.png_file_bytes(h, w, STRIP_ROWS) == cap + 57
    with pytest.raises(Exception):                                     # a slot below the bound is refused on the host
        wrap(shape, "scene", False, file_cap=cap + 56)
    with pytest.raises(Exception):
        wrap(shape, "scene", True, file_cap=ops.apng_file_bytes(n, h, w, STRIP_ROWS) - 1)
    with pytest.raises(Exception):
        wrap(shape, "scene", False, ws_short=8)
    with pytest.raises(Exception):
        wrap(shape, "scene", True, ws_short=8)
    for delay in ((0, 7), (65536, 7), (1, 65536), (1, -1)):
        with pytest.raises(Exception):
            wrap(shape, "scene", True, delay=delay)
    wrap(shape, "scene", True, delay=(65535, 0))                       # and these are taken
    wrap(shape, "scene", False, delay=(0, 0))                          # (a still has no delay)
    for bad in ("gpu", "", None, True):
        with pytest.raises(ValueError):
            PngEncoder(DEV, h, w, assemble=bad)
    with pytest.raises(ValueError):
        PngEncoder(DEV, h, w).encode_apng(torch.zeros((1, h, w, 3), dtype=torch.uint8, device=DEV), fps=0)


# ---------------------------------------------------------------------------------------------------- call site
def test_frame_emitter_png_output_is_the_host_routes_files():
    pytest.importorskip("PIL.Image")
    from vdpp_amd.models.edge_stages import FrameEmitter, decode_latents_uint8
    from vdpp_amd.models.image_io import PngEncoder
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
    model.set_dummy_conditioning(1, 3, 8, 16, dev)
    spec = LatentSpec(shape=torch.Size((1, 4, 3, 8, 16)), dtype=torch.float16, device=dev)

    def supplier(i):
        g = torch.Generator().manual_seed(1000 + i)
        return (torch.randn(spec.shape, generator=g) * model.init_noise_sigma).half().to(dev)

    stage = PipelineStage(model, PipelineConfig(total_steps=2, timesteps=[0, 1], world_size=1, rank=0, latent_spec=spec))
    emitter = FrameEmitter(decoder, stage, 3, output="png")
    with torch.no_grad():
        out = stage.run_many(2, input_supplier=supplier)
        stage.drain()
        files = emitter.finish(2)
        assert emitter._jpeg.assemble == "device" and sorted(files) == [0, 1]
        host = PngEncoder(DEV, 64, 128, assemble="host")
        for i in range(2):
            u8 = decode_latents_uint8(out[i].contiguous(), decoder, 3)
            assert isinstance(files[i], list) and len(files[i]) == 1 and len(files[i][0]) == 3
            assert files[i][0] == host.encode(u8[0])
            for k in range(3):
                size, _, pictures = decode(files[i][0][k])
                assert size == (128, 64) and np.array_equal(pictures[0], u8[0][k].cpu().numpy())
