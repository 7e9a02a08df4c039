"""Image front end and 8-bit frame output, the parts that need no GPU: the geometry rules against what the real functions
do (tests/golden/image_io.npz, minted by tests/golden/make_image_golden.py from the reference's
``load_and_preprocess_image``, Pillow and transformers), the fixture against a fresh mint (version drift), the C ABI's
argument checks, and the frame writers."""

import ctypes
import os

import numpy as np
import pytest

from vdpp_amd import hip


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "image_io.npz"))


def test_cover_geometry_is_the_reference_rule(golden):
    from vdpp_amd.models.image_io import cover_geometry
    pairs, want = golden["cover_pairs"], golden["cover_geometry"]
    assert len(pairs) >= 40
    for p, w in zip(pairs.tolist(), want.tolist()):
        assert list(cover_geometry(*p)) == w, p
    # Python's round is half to even: both directions are in the table
    assert list(cover_geometry(101, 200, 50, 100))[:2] == [50, 100] and list(cover_geometry(103, 200, 50, 100))[:2] == [52, 100]


def test_clip_geometry_is_the_processors_rule(golden):
    from vdpp_amd.models.image_io import clip_geometry
    pairs, want = golden["clip_pairs"], golden["clip_geometry"]
    assert len(pairs) >= 40
    for p, w in zip(pairs.tolist(), want.tolist()):
        assert list(clip_geometry(*p)) == w, p
    assert clip_geometry(576, 1024, 224) == (224, 398, 0, 87)


def test_fixture_equals_a_fresh_mint(golden):
    """Everything in the stored fixture, minted again in memory by the installed Pillow / transformers through the
    reference's own function: a version whose resize or processor differs shows here, not as a GPU failure."""
    pytest.importorskip("PIL")
    pytest.importorskip("transformers")
    from tests.golden import make_image_golden as mint
    if not os.path.exists(mint.REFERENCE_SCRIPT):
        pytest.skip("the reference's script is not on this machine")
    fresh = mint.build()
    assert sorted(fresh) == sorted(golden.files)
    for key in golden.files:
        a, b = golden[key], np.asarray(fresh[key])
        assert a.shape == b.shape and a.dtype == b.dtype, key
        assert np.array_equal(a, b), key
    assert float(golden["raw_model_share"].max()) <= mint.MAX_MODEL_SHARE
    assert float(golden["chain_model_share"].max()) <= mint.MAX_MODEL_SHARE


def test_source_images_are_the_minted_ones(golden):
    """The sources are regenerated from seeds, not stored: their CRCs are."""
    from tests.golden import make_image_golden as mint
    for i, ((sh, sw), _, _) in enumerate(mint.RAW_CASES):
        for j, kind in enumerate(mint.KINDS):
            assert mint.crc(mint.source_image(kind, sh, sw, mint.case_seed(0, i, kind))) == int(golden["raw_source_crc"][i, j])
    for i, ((sh, sw), kind) in enumerate(mint.CHAIN_CASES):
        assert mint.crc(mint.source_image(kind, sh, sw, mint.case_seed(1, i, kind))) == int(golden["chain_source_crc"][i])


def test_new_entry_points_reject_bad_arguments_without_launching():
    lib = hip.load()
    for name in ("sp_image_resample_tmp_bytes", "sp_image_resample_u8", "sp_image_to_tensor_f16", "sp_frames_to_u8",
                 "sp_vae_frames_out_u8"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert lib.sp_image_resample_tmp_bytes(37, 109) == 37 * 109 * 3
    assert lib.sp_image_resample_tmp_bytes(0, 5) == 0
    buf = ctypes.create_string_buffer(4096)          # host memory: every call below must be refused before any launch
    p = ctypes.addressof(buf)
    ok = dict(src=p, sp=30, sh=4, sw=10, dst=p, dp=15, dh=2, dw=5, filt=1, tmp=p, tb=4 * 5 * 3)

    def resample(**kw):
        a = dict(ok, **kw)
        return lib.sp_image_resample_u8(a["src"], a["sp"], a["sh"], a["sw"], a["dst"], a["dp"], a["dh"], a["dw"], a["filt"],
                                        a["tmp"], a["tb"], None)

    for bad, word in ((dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(tmp=None), b"null"), (dict(sh=0), b"positive"),
                      (dict(dw=0), b"positive"), (dict(tb=4 * 5 * 3 - 1), b"tmp"), (dict(filt=2), b"filter"),
                      (dict(filt=-1), b"filter"), (dict(sp=29), b"pitch"), (dict(dp=14), b"pitch")):
        assert resample(**bad) == -1, bad
        assert word in lib.sp_last_error(), (bad, lib.sp_last_error())
    m = (0.5, 0.5, 0.5)
    assert lib.sp_image_to_tensor_f16(None, 30, 4, 10, p, *m, *m, None) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_image_to_tensor_f16(p, 30, 4, 10, None, *m, *m, None) == -1
    assert lib.sp_image_to_tensor_f16(p, 30, 0, 10, p, *m, *m, None) == -1
    assert lib.sp_image_to_tensor_f16(p, 29, 4, 10, p, *m, *m, None) == -1 and b"pitch" in lib.sp_last_error()
    assert lib.sp_image_to_tensor_f16(p, 30, 4, 10, p, *m, 0.5, 0.0, 0.5, None) == -1
    assert lib.sp_frames_to_u8(None, 1, p, 1, 1, 2, 2, None) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_frames_to_u8(p, 1, None, 1, 1, 2, 2, None) == -1
    assert lib.sp_frames_to_u8(p, 1, p, 1, 0, 2, 2, None) == -1
    assert lib.sp_vae_frames_out_u8(None, 8, p, p, p, 1, 1, 2, 2, 0, None) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_vae_frames_out_u8(p, 8, p, p, None, 1, 1, 2, 2, 0, None) == -1
    assert lib.sp_vae_frames_out_u8(p, 6, p, p, p, 1, 1, 2, 2, 0, None) == -1
    assert lib.sp_vae_frames_out_u8(p, 8, p, p, p, 1, 0, 2, 2, 0, None) == -1
    assert lib.sp_vae_frames_out_u8(p, 8, p, p, p, 1, 1, 2, 2, -1, None) == -1


def _frames():
    f = np.zeros((3, 10, 16, 3), np.uint8)
    for i in range(3):
        f[i, :, :, 0] = 80 * i + 10
        f[i, 2 * i:2 * i + 4, 3:9, 1] = 255
        f[i, :, :, 2] = np.arange(16)[None, :] * 16
    return f


def test_save_frames_round_trips_gif_and_pngs(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.models.image_io import load_image, save_frames
    f = _frames()
    files = save_frames(f, str(tmp_path / "v.gif"), fps=5)
    assert files == [str(tmp_path / "v.gif")]
    with Image.open(files[0]) as im:
        assert im.n_frames == 3 and im.size == (16, 10)
        assert im.info.get("loop") == 0 and im.info.get("duration") == 200
        for i in range(3):                      # GIF is palettised: few colours here, so the round trip is exact
            im.seek(i)
            assert np.array_equal(np.asarray(im.convert("RGB")), f[i]), i
    for target, names in ((tmp_path / "frames", ["000.png", "001.png", "002.png"]),
                          (tmp_path / "f_%03d.png", ["f_000.png", "f_001.png", "f_002.png"])):
        files = save_frames(f, str(target), fps=5)
        assert [os.path.basename(n) for n in files] == names
        for i, name in enumerate(files):
            assert np.array_equal(load_image(name), f[i])
    files = save_frames(f, str(tmp_path / "v.npy"))
    assert np.array_equal(np.load(files[0]), f)


def test_save_frames_refuses_what_it_cannot_write(tmp_path):
    from vdpp_amd.models.image_io import save_frames
    with pytest.raises(ValueError, match="imageio / ffmpeg"):
        save_frames(_frames(), str(tmp_path / "v.mp4"))
    assert not (tmp_path / "v.mp4").exists()
    with pytest.raises(ValueError, match="pattern"):
        save_frames(_frames(), str(tmp_path / "single.png"))
    with pytest.raises(ValueError):
        save_frames(_frames().astype(np.float32), str(tmp_path / "v.gif"))


@pytest.fixture
def host_encoders(monkeypatch):
    """The four frame encoders built for 16 x 24 frames with the device check replaced: what they refuse, they refuse before
    anything is launched."""
    import torch
    from vdpp_amd.models import common, image_io
    monkeypatch.setattr(common, "hip_device", lambda device, engine: torch.device(device))
    return [cls("cpu", 16, 24) for cls in (image_io.JpegEncoder, image_io.GifEncoder, image_io.PngEncoder, image_io.WebpEncoder)]


def test_encoders_refuse_other_frames_with_one_message(host_encoders):
    import torch
    good = torch.zeros((2, 16, 24, 3), dtype=torch.uint8)
    cases = ((good.float(), "torch.float32 (2, 16, 24, 3)"), (good[0], "torch.uint8 (16, 24, 3)"),
             (good[:, :, :23], "torch.uint8 (2, 16, 23, 3)"), (good[:, :15], "torch.uint8 (2, 15, 24, 3)"),
             (torch.zeros((2, 16, 24, 4), dtype=torch.uint8), "torch.uint8 (2, 16, 24, 4)"),
             (good[:0], "torch.uint8 (0, 16, 24, 3)"), (good.numpy(), "uint8 (2, 16, 24, 3)"), ([[1, 2, 3]], "<class 'list'> ()"))
    for enc in host_encoders:
        for frames, got in cases:
            with pytest.raises(ValueError) as refused:
                enc.enqueue(frames)
            assert str(refused.value) == f"frames must be a (F, 16, 24, 3) uint8 tensor; got {got}", type(enc).__name__
        for name in ("encode",) + (("enqueue_files", "encode_apng") if hasattr(enc, "encode_apng") else ()) \
                + (("encode_animation",) if hasattr(enc, "encode_animation") else ()):
            with pytest.raises(ValueError, match="frames must be a"):
                getattr(enc, name)(good.float())


def test_write_apng_and_the_device_route_refuse_the_same_fps(host_encoders):
    from vdpp_amd.models.image_io import write_apng
    png = host_encoders[2]
    for fps in (0, -1, 0.0, float("nan"), True, "7", None, 1e-6, 1 / 70000):
        with pytest.raises(ValueError) as host:
            write_apng(None, [b"x"], 24, 16, fps)
        with pytest.raises(ValueError) as device:
            png.enqueue_apng(None, fps)                      # (the delay is worked out before the frames are looked at)
        if "delay" in str(device.value):
            assert str(device.value) == f"a delay of 1 / {fps} s does not fit the frame control chunk"
            assert str(host.value) == "write_apng: " + str(device.value)
        else:
            assert str(host.value) == str(device.value) == f"fps must be a positive number; got {fps!r}"
    for fps in (7, 12.5, 1 / 3, 1 / 65535, 65535, np.float32(24)):
        assert write_apng(None, [b"x"], 24, 16, fps)[:8] == b"\x89PNG\r\n\x1a\n"
        with pytest.raises(ValueError, match="frames must be a"):
            png.enqueue_apng(None, fps)


def test_generate_mode_names_and_flags():
    from vdpp_amd.modes import generate
    assert generate.sample_output_path("out.gif", 0, 1) == "out.gif"
    assert generate.sample_output_path("out.gif", 2, 3) == "out_s2.gif"
    assert generate.sample_output_path("frames", 1, 2) == "frames_s1"
    a = generate.parse_args(["--random-init", "--input-image", "in.png", "--output", "out.gif"])
    assert (a.height, a.width, a.num_frames, a.num_samples) == (576, 1024, 14, 1)
    for bad in (["--input-image", "in.png", "--output", "o.gif"],                                   # neither weights source
                ["--random-init", "--model-id", "x", "--input-image", "in.png", "--output", "o.gif"],
                ["--random-init", "--height", "60", "--input-image", "in.png", "--output", "o.gif"]):
        with pytest.raises(SystemExit):
            generate.parse_args(bad)
