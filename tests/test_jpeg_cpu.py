"""Video files out, the parts that need no GPU: the tables and the header of the JPEG frames against Pillow (libjpeg),
the AVI container against a strict RIFF walker, the new targets of save_frames / generate, and the refusals of the C ABI.
tests/jpeg_model.py is the independent statement of the encoder the header is tried with."""

import ctypes
import io
import struct
import warnings

import numpy as np
import pytest

from tests import jpeg_model as jm

Image = pytest.importorskip("PIL.Image")


def _pillow_jpeg(frame, quality):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def _decode(data):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            return im.mode, im.size, np.asarray(im.convert("RGB"))


def _segments(data):
    """marker -> list of payloads, up to SOS."""
    at, out = 2, {}
    while data[at + 1] != 0xDA:
        assert data[at] == 0xFF
        size = struct.unpack(">H", data[at + 2:at + 4])[0]
        out.setdefault(data[at + 1], []).append(data[at + 4:at + 2 + size])
        at += 2 + size
    return out


@pytest.mark.parametrize("quality", [1, 30, 50, 75, 90, 100])
def test_quant_tables_are_libjpegs(quality):
    from vdpp_amd.hip import ops
    luma, chroma = ops.jpeg_quant_tables(quality)
    with Image.open(io.BytesIO(_pillow_jpeg(jm.noise_frames(1, 16, 16, 0)[0], quality))) as im:
        theirs = im.quantization
    for ours, model, got in ((luma, jm.quant_tables(quality)[0], theirs[0]), (chroma, jm.quant_tables(quality)[1], theirs[1])):
        assert sorted(ours) == sorted(got)
        assert list(ours) == model.tolist()
        # Pillow reports a table either as the file holds it (zigzag) or put back in natural order, by version
        assert list(got) in (list(ours), [ours[i] for i in jm.ZIGZAG])


def test_huffman_tables_are_libjpegs_defaults():
    from vdpp_amd.hip import ops
    theirs = {}
    for payload in _segments(_pillow_jpeg(jm.noise_frames(1, 16, 16, 0)[0], 90))[0xC4]:
        while payload:                                             # a DHT segment may hold several tables
            n = sum(payload[1:17])
            theirs[payload[0]] = (list(payload[1:17]), list(payload[17:17 + n]))
            payload = payload[17 + n:]
    for which, tc_th in ((0, 0x00), (1, 0x01), (2, 0x10), (3, 0x11)):
        bits, vals = ops.jpeg_huffman_table(which)
        assert (list(bits), list(vals)) == theirs[tc_th]
        assert (list(bits), list(vals)) == (jm.HUFFMAN_SPECS[which][0], jm.HUFFMAN_SPECS[which][1])


@pytest.mark.parametrize("h,w,restart,quality,kind", [(50, 37, 3, 90, "scene"), (48, 80, 5, 50, "noise"), (16, 16, 1, 100, "noise"),
                                                       (64, 96, 7, 75, "scene")])
def test_header_plus_the_models_scan_is_a_file_pillow_decodes(h, w, restart, quality, kind):
    """jpeg_header + the model's entropy-coded segment + EOI: Pillow opens it without a warning at the right size, and what
    it decodes is as close to the original as Pillow's own encode at that quality (within 0.05 dB)."""
    from vdpp_amd.models.image_io import jpeg_header
    frame = (jm.scene_frames if kind == "scene" else jm.noise_frames)(1, h, w, 5)
    coef, _, _ = jm.coefficients(frame, quality)
    scan, _ = jm.entropy_segment(coef[0], restart)
    data = jpeg_header(h, w, quality, restart) + scan + b"\xff\xd9"
    mode, size, got = _decode(data)
    assert mode == "RGB" and size == (w, h)
    ours, theirs = jm.psnr(got, frame[0]), jm.psnr(_decode(_pillow_jpeg(frame[0], quality))[2], frame[0])
    print(f"{h}x{w} q{quality} {kind}: {ours:.3f} dB, Pillow {theirs:.3f} dB")
    assert ours >= theirs - 0.05
    seg = _segments(data)
    assert seg[0xDD] == [struct.pack(">H", restart)]
    assert struct.unpack(">BHHB", seg[0xC0][0][:6]) == (8, h, w, 3) and seg[0xC0][0][6:] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])


def test_header_refuses_what_a_frame_cannot_say():
    from vdpp_amd.models.image_io import jpeg_header
    for bad in ((0, 16, 90, 1), (16, 65536, 90, 1), (16, 16, 0, 1), (16, 16, 101, 1), (16, 16, 90, 0), (16, 16, 90, 65536)):
        with pytest.raises(ValueError):
            jpeg_header(*bad)


def _frames(n=4, h=24, w=40):
    return jm.scene_frames(n, h, w, 11)


def _check_avi(data, jpegs, w, h, fps):
    res = jm.walk_avi(data)
    assert res["lists"] == [b"hdrl", b"strl", b"movi"]
    avih = res["avih"]
    assert avih[0] == 1000000 // fps and avih[3] & 0x10 and avih[4] == len(jpegs) and avih[6] == 1 and avih[8:10] == (w, h)
    strh = struct.unpack("<4s4sIHHIIIIIIIIHHHH", res["strh"])
    assert strh[:2] == (b"vids", b"MJPG") and strh[6:8] == (1, fps) and strh[9] == len(jpegs) and strh[-2:] == (w, h)
    strf = struct.unpack("<IiiHH4sIiiII", res["strf"])
    assert strf[:6] == (40, w, h, 1, 24, b"MJPG")
    assert res["frames"] == list(jpegs)
    assert len(res["index"]) == len(jpegs)
    for (ckid, flags, off, size), at, j in zip(res["index"], res["frame_offsets"], jpegs):
        assert ckid == b"00dc" and flags & 0x10 and off == at and size == len(j)
    for j in res["frames"]:
        assert j[:2] == b"\xff\xd8" and j.rstrip(b"\0")[-2:] == b"\xff\xd9"
    return res


def test_write_avi_is_a_consistent_riff_file(tmp_path):
    from vdpp_amd.models.image_io import write_avi
    frames = _frames()
    jpegs = [_pillow_jpeg(f, 85) for f in frames]
    if not any(len(j) & 1 for j in jpegs):
        jpegs[1] += b"\0"                                          # a byte after EOI: decoders stop at EOI
    assert any(len(j) & 1 for j in jpegs) and any(not len(j) & 1 for j in jpegs)
    path = tmp_path / "v.avi"
    write_avi(str(path), jpegs, 40, 24, 7)
    data = path.read_bytes()
    res = _check_avi(data, jpegs, 40, 24, 7)
    for j, f in zip(res["frames"], frames):
        mode, size, got = _decode(j)
        assert size == (40, 24) and np.array_equal(got, _decode(_pillow_jpeg(f, 85))[2])
    for bad in (dict(jpegs=[]), dict(fps=0), dict(width=0)):
        kw = dict(jpegs=jpegs, width=40, height=24, fps=7)
        kw.update(bad)
        with pytest.raises(ValueError):
            write_avi(str(tmp_path / "bad.avi"), **kw)
    assert not (tmp_path / "bad.avi").exists()


def test_write_avi_refuses_two_gib(tmp_path):
    """32 references to one 64 MiB frame: the size is refused from the lengths, before anything is put together."""
    from vdpp_amd.models.image_io import write_avi
    blob = _pillow_jpeg(_frames(1)[0], 85) + bytes(2 ** 26)
    with pytest.raises(ValueError, match="2 GiB"):
        write_avi(str(tmp_path / "big.avi"), [blob] * 32, 40, 24, 7)
    assert not (tmp_path / "big.avi").exists()


def test_save_frames_avi_and_jpeg_pattern_from_host_memory(tmp_path):
    from vdpp_amd.models.image_io import save_frames
    frames = _frames()
    jpegs = [_pillow_jpeg(f, 80) for f in frames]
    assert save_frames(frames, str(tmp_path / "v.avi"), fps=5, quality=80) == [str(tmp_path / "v.avi")]
    _check_avi((tmp_path / "v.avi").read_bytes(), jpegs, 40, 24, 5)
    import torch
    files = save_frames(torch.from_numpy(frames), str(tmp_path / "f_%03d.jpg"))
    assert files == [str(tmp_path / f"f_{i:03d}.jpg") for i in range(4)]
    for name, f in zip(files, frames):
        assert open(name, "rb").read() == _pillow_jpeg(f, 90)
    assert len(save_frames(frames, str(tmp_path / "g_%02d.jpeg"), quality=30)) == 4
    with pytest.raises(ValueError, match="imageio / ffmpeg"):
        save_frames(frames, str(tmp_path / "v.mp4"))
    with pytest.raises(ValueError, match=r"write \.avi \(Motion-JPEG\) instead"):
        save_frames(frames, str(tmp_path / "v.mp4"))
    assert not (tmp_path / "v.mp4").exists()
    for q in (0, 101):
        for name in ("q.avi", "q_%03d.jpg"):
            with pytest.raises(ValueError, match="quality"):
                save_frames(frames, str(tmp_path / name), quality=q)
    with pytest.raises(ValueError, match="pattern"):
        save_frames(frames, str(tmp_path / "single.jpg"))
    assert not list(tmp_path.glob("q*")) and not (tmp_path / "single.jpg").exists()


def test_generate_takes_a_jpeg_quality():
    from vdpp_amd.modes import generate
    base = ["--random-init", "--input-image", "in.png", "--output", "out.avi"]
    assert generate.parse_args(base).jpeg_quality == 90
    assert generate.parse_args(base + ["--jpeg-quality", "80"]).jpeg_quality == 80
    for bad in ("0", "101"):
        with pytest.raises(SystemExit):
            generate.parse_args(base + ["--jpeg-quality", bad])


def test_abi_refuses_bad_jpeg_arguments_before_any_launch():
    from vdpp_amd import hip
    lib = hip.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    lu, ch = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
    assert lib.sp_jpeg_quant_tables(0, ctypes.addressof(lu), ctypes.addressof(ch)) == -1 and b"quality" in lib.sp_last_error()
    assert lib.sp_jpeg_quant_tables(101, ctypes.addressof(lu), ctypes.addressof(ch)) == -1
    assert lib.sp_jpeg_quant_tables(50, None, ctypes.addressof(ch)) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_jpeg_huffman_table(4, p, p) == -1 and lib.sp_jpeg_huffman_table(0, None, p) == -1
    # coefficient stage: null pointers, quality 0 / 101, h or w of 0
    assert lib.sp_jpeg_dct_quant_u8(None, 1, 16, 16, 90, p, None) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_jpeg_dct_quant_u8(p, 1, 16, 16, 90, None, None) == -1
    assert lib.sp_jpeg_dct_quant_u8(p, 1, 16, 16, 0, p, None) == -1 and b"quality" in lib.sp_last_error()
    assert lib.sp_jpeg_dct_quant_u8(p, 1, 16, 16, 101, p, None) == -1
    assert lib.sp_jpeg_dct_quant_u8(p, 1, 0, 16, 90, p, None) == -1
    assert lib.sp_jpeg_dct_quant_u8(p, 1, 16, 0, 90, p, None) == -1
    assert lib.sp_jpeg_dct_quant_u8(p, 0, 16, 16, 90, p, None) == -1
    assert lib.sp_jpeg_coef_bytes(3, 50, 37) == 3 * 4 * 3 * 6 * 64 * 2 and lib.sp_jpeg_coef_bytes(1, 0, 16) == 0
    # entropy stage
    cap = lib.sp_jpeg_stream_bytes(48, 80, 5)
    assert cap == 416 * 6 * 15 + 2 * 2 and lib.sp_jpeg_stream_bytes(48, 80, 1) == 416 * 6 * 15 + 2 * 14
    assert lib.sp_jpeg_stream_bytes(48, 80, 0) == 0 and lib.sp_jpeg_stream_bytes(48, 80, 65536) == 0
    assert lib.sp_jpeg_stream_bytes(0, 80, 5) == 0 and lib.sp_jpeg_stream_bytes(48, 0, 5) == 0
    ws = lib.sp_jpeg_entropy_ws_bytes(2, 3, 5, 5)
    assert ws == 256 + 2 * 3 * 416 * 6 * 5 and lib.sp_jpeg_entropy_ws_bytes(2, 3, 5, 0) == 0
    good = [p, 2, 3, 5, 5, p, cap, p, p, ws, None]

    def refused(word, **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        assert lib.sp_jpeg_entropy(*args) == -1
        assert word in lib.sp_last_error(), lib.sp_last_error()

    for i in (0, 5, 7, 8):
        refused(b"null", **{f"a{i}": None})
    refused(b"restart_mcus", a4=0)
    refused(b"restart_mcus", a4=65536)
    refused(b"cap", a6=cap - 1)
    refused(b"ws", a9=ws - 1)
    refused(b"mcu", a2=0)
    refused(b"mcu", a3=0)
    refused(b"n must be positive", a1=0)
