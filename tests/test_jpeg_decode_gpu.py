"""The device JPEG decoder (csrc/jpeg_decode.hip) on the GPU, against tests/jpeg_decode_model.py: coefficients, pixels and the
count of synchronisation passes on every fixture of the model's table, JpegEncoder's own files back in, and the picture
input of the generate mode.  Every file here is a valid one: damaged streams are decoded only on the host
(tests/test_jpeg_decode_cpu.py, under the sanitizers).

The model's pixels equal Pillow's on every fixture (profiles/jpeg_decode_parity.txt: max |diff| 0), so equality with the
model passes on the bound of 4 levels against Pillow that the decoder is held to."""

import ctypes
import io

import numpy as np
import pytest
import torch

from tests import jpeg_decode_model as model
from tests import jpeg_model

pytestmark = pytest.mark.gpu

NAMES = list(model.fixtures())


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", NAMES)
def test_fixture_decodes_to_the_models_coefficients_and_pixels(dev, name):
    from vdpp_amd.models import image_io

    data, subseq_bits = model.fixtures()[name]
    coef, passes, px = model.expected(name)
    dec = image_io.JpegDecoder(dev, subseq_bits=subseq_bits)
    rgb = dec.decode(data)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == px.shape and rgb.device.type == "cuda"
    status = dec.last_status
    assert status[0] == 0 and status[10] == 1, status
    assert np.array_equal(dec.last_coef.cpu().numpy(), coef)
    assert np.array_equal(rgb.cpu().numpy(), px)
    assert dec.last_passes == passes, "the count of passes is a function of the file, and the model's"
    # one pass per round: the status word is read after each, and further rounds are enqueued until the fixed point
    one = image_io.JpegDecoder(dev, subseq_bits=subseq_bits, sync_passes=1)
    again = one.decode(data)
    assert one.last_passes == passes and one.last_status[10] == 1
    assert torch.equal(again, rgb) and np.array_equal(one.last_coef.cpu().numpy(), coef)


def test_a_decoder_is_reused_across_sizes_and_results_are_fresh_tensors(dev):
    from vdpp_amd.models import image_io

    dec = image_io.JpegDecoder(dev)
    first = dec.decode(model.fixtures()["scene144x256_q90"][0])
    second = dec.decode(model.fixtures()["noise37x51_422"][0])
    third = dec.decode(model.fixtures()["scene144x256_q90"][0])
    assert np.array_equal(first.cpu().numpy(), model.expected("scene144x256_q90")[2])
    assert np.array_equal(second.cpu().numpy(), model.expected("noise37x51_422")[2])
    assert torch.equal(first, third) and first.data_ptr() != third.data_ptr()


@pytest.mark.parametrize("kind,h,w,quality,restart", [("scene", 40, 72, 90, None), ("noise", 37, 51, 75, 1), ("scene", 48, 64, 50, 7)])
def test_the_encoders_own_files_come_back(dev, kind, h, w, quality, restart):
    from vdpp_amd.models import image_io

    frames = (jpeg_model.noise_frames if kind == "noise" else jpeg_model.scene_frames)(2, h, w, 31)
    enc = image_io.JpegEncoder(dev, h, w, quality=quality, restart_mcus=restart)
    files = enc.encode(torch.from_numpy(frames).to(dev))
    want = enc._buf("coef", (2, enc.mcu_rows, enc.mcu_cols, 6, 64), torch.int16).cpu().numpy()       # ops.jpeg_dct_quant's buffer
    dec = image_io.JpegDecoder(dev)
    for i, data in enumerate(files):
        rgb = dec.decode(data).cpu().numpy()
        assert np.array_equal(dec.last_coef.cpu().numpy(), want[i]), "decoded coefficients are not the encoder's"
        ref = model.pillow_pixels(data)
        # parity with Pillow is measured at max |diff| 0, mean 0: the same PSNR against the source, to rounding of the logarithm
        assert abs(jpeg_model.psnr(rgb, frames[i]) - jpeg_model.psnr(ref, frames[i])) < 1e-9
        assert np.abs(rgb.astype(int) - ref.astype(int)).max() <= 4


def test_load_image_device_feeds_the_front_end(dev, tmp_path):
    from PIL import Image

    from vdpp_amd.models import image_io

    picture = jpeg_model.scene_frames(1, 96, 160, 41)[0]
    Image.fromarray(picture).save(tmp_path / "in.jpg", quality=92)
    Image.fromarray(picture).save(tmp_path / "in.png")
    Image.fromarray(picture).save(tmp_path / "progressive.jpg", quality=92, progressive=True)
    front = image_io.ImageFrontEnd(dev, 64, 128, clip_size=32)
    for name in ("in.jpg", "in.png", "progressive.jpg"):
        got = image_io.load_image_device(str(tmp_path / name), dev)
        assert got.is_cuda and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), image_io.load_image(str(tmp_path / name))), name
        pixel_values, image_tensor, crop = front(got)
        host = front(image_io.load_image(str(tmp_path / name)))
        assert torch.equal(pixel_values, host[0]) and torch.equal(image_tensor, host[1]) and torch.equal(crop, host[2])


def test_generate_decodes_its_picture_on_the_device(monkeypatch, tmp_path, dev):
    from PIL import Image

    from vdpp_amd.modes import generate

    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    src = tmp_path / "in.jpg"
    Image.fromarray(jpeg_model.scene_frames(1, 80, 150, 42)[0]).save(src, quality=92)

    def run(out, tag, decode):
        generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_{tag}", "--log-level", "WARNING",
                       "--random-init", "--tiny", "--input-image", str(src), "--height", "64", "--width", "128",
                       "--num-frames", "3", "--total-steps", "2", "--output", str(out)] + decode)
        assert not torch.distributed.is_initialized()

    run(tmp_path / "device.npy", "a", ["--input-decode", "device"])
    a = np.load(tmp_path / "device.npy")
    assert a.shape == (3, 64, 128, 3) and a.dtype == np.uint8 and int(a.max()) > int(a.min())
    run(tmp_path / "host.npy", "b", [])
    assert np.array_equal(a, np.load(tmp_path / "host.npy")), "the device decode gave another picture than Pillow's"
    assert generate.parse_args(["--input-image", "x", "--output", "y.npy", "--random-init"]).input_decode == "host"


def test_bad_arguments_return_minus_one_without_launching(dev):
    from vdpp_amd import hip
    from vdpp_amd.hip import ops
    from vdpp_amd.models import image_io

    lib = hip.load()
    info = image_io.parse_jpeg(model.fixtures()["noise8x8_420"][0])
    host = ops.jpeg_decode_plan(info.plan_fields(1024), *info.plan_tables())
    plan = ops.JpegPlan(host, torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev))
    ws = torch.zeros(plan.ws_bytes, dtype=torch.uint8, device=dev)
    seg = torch.zeros(info.segment_length, dtype=torch.uint8, device=dev)
    coef = torch.zeros(plan.coef_bytes // 2, dtype=torch.int16, device=dev)
    assert plan.ws_bytes > 0 and plan.coef_bytes == 6 * 64 * 2
    args = (plan.ptr, plan.dev.data_ptr())
    assert lib.sp_jpeg_decode_split(*args, seg.data_ptr(), ws.data_ptr(), plan.ws_bytes - 1, None) == -1
    assert b"sp_jpeg_decode_ws_bytes" in lib.sp_last_error()
    assert lib.sp_jpeg_decode_split(*args, None, ws.data_ptr(), plan.ws_bytes, None) == -1
    assert lib.sp_jpeg_decode_split(*args, seg.data_ptr(), ws.data_ptr() + 4, plan.ws_bytes, None) == -1
    assert lib.sp_jpeg_decode_sync(*args, ws.data_ptr(), plan.ws_bytes, 0, 0, None) == -1
    assert lib.sp_jpeg_decode_sync(*args, ws.data_ptr(), plan.ws_bytes, -1, 1, None) == -1
    assert lib.sp_jpeg_decode_sync(*args, ws.data_ptr(), plan.ws_bytes, 0, 5000, None) == -1
    assert lib.sp_jpeg_decode_coefficients(*args, ws.data_ptr(), plan.ws_bytes, 0, None, None) == -1
    assert lib.sp_jpeg_decode_coefficients(*args, ws.data_ptr(), plan.ws_bytes, -1, coef.data_ptr(), None) == -1
    assert lib.sp_jpeg_decode_pixels(*args, ws.data_ptr(), plan.ws_bytes, coef.data_ptr(), None, None) == -1
    junk = ctypes.create_string_buffer(len(host))
    assert lib.sp_jpeg_decode_sync(ctypes.addressof(junk), plan.dev.data_ptr(), ws.data_ptr(), plan.ws_bytes, 0, 1, None) == -1
    torch.cuda.synchronize()
    assert not ws.any(), "a refused call wrote to its scratch"
    with pytest.raises(ValueError, match="subseq_bits"):
        image_io.JpegDecoder(dev, subseq_bits=100)
    with pytest.raises(ValueError, match="sync_passes"):
        image_io.JpegDecoder(dev, sync_passes=0)
