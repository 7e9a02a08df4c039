"""The device JPEG decoder without a GPU: the header parser, the model (tests/jpeg_decode_model.py) against the encoder's model
and against Pillow, the pass scheme against the serial decode, and the functions the kernels are made of
(csrc/jpeg_decode_core.h) run serially by tools/jpeg_decode_hostcheck.cpp under the host sanitizers, on the fixtures and on
damaged copies of them.  No malformed stream is decoded anywhere else.

Model against Pillow: a conforming inverse DCT is within one level of another, the same triangle filter keeps that, and the
colour conversion multiplies a chrominance error by at most 1.772 and rounds once: max |diff| <= 4.  The model restates
libjpeg's own integer arithmetic, so the measured difference is 0 on every fixture (profiles/jpeg_decode_parity.txt)."""

import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_model as model
from tests import jpeg_model
from vdpp_amd.hip import ops
from vdpp_amd.models import image_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "jpeg_decode_parity.txt")
NAMES = list(model.fixtures())


def _pillow_jpeg(array, **options):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(array).save(buf, format="JPEG", **options)
    return buf.getvalue()


# ------------------------------------------------------------------------------------------------ header parsing
@pytest.mark.parametrize("name", NAMES)
def test_parse_jpeg_reads_the_fixture(name):
    data = model.fixtures()[name][0]
    info, want = image_io.parse_jpeg(data), model.parse(data)
    assert (info.width, info.height, info.components, info.hs, info.vs) == (want.width, want.height, want.ncomp, want.hs, want.vs)
    assert info.tq == tuple(c[3] for c in want.comps) and info.td == tuple(want.td) and info.ta == tuple(want.ta)
    assert info.restart_interval == want.restart
    assert (info.segment_offset, info.segment_length) == (want.start, want.end - want.start)
    assert data[info.segment_offset + info.segment_length:] == b"\xff\xd9"
    assert set(info.quant) == set(want.quant) and all(np.array_equal(info.quant[k], want.quant[k]) for k in want.quant)
    assert {k: (list(b), list(v)) for k, (b, v) in info.dht.items()} == want.dht
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        assert im.size == (info.width, info.height)


def test_the_q100_fixtures_hold_stuffed_bytes():
    for name in NAMES:
        if "_q100_" in name:
            data = model.fixtures()[name][0]
            info = image_io.parse_jpeg(data)
            seg = data[info.segment_offset:info.segment_offset + info.segment_length]
            assert seg.count(b"\xff\x00") >= 8, name


def test_the_restart_fixtures_hold_what_they_are_for():
    info = image_io.parse_jpeg(model.fixtures()["noise37x51_420_rst1"][0])
    assert info.restart_interval == 1 and model.parse(model.fixtures()["noise37x51_420_rst1"][0]).n_iv == 12   # RSTn wraps past 7
    h = model.parse(model.fixtures()["noise37x51_420_rst5"][0])
    assert h.interval == 5 and h.total_mcus % 5 == 2                                                            # a short last interval


def test_parse_jpeg_refuses_what_is_out_of_scope():
    rgb = jpeg_model.scene_frames(1, 24, 40, 3)[0]
    with pytest.raises(image_io.UnsupportedJpeg, match="progressive"):
        image_io.parse_jpeg(_pillow_jpeg(rgb, quality=90, progressive=True))
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(buf, format="JPEG", quality=90)
    with pytest.raises(image_io.UnsupportedJpeg, match="four components"):
        image_io.parse_jpeg(buf.getvalue())
    with pytest.raises(image_io.UnsupportedJpeg, match="sampling factors"):
        image_io.parse_jpeg(_resample(_pillow_jpeg(rgb, quality=90, subsampling=0), 0x12))            # 4:4:0
    assert issubclass(image_io.UnsupportedJpeg, ValueError)


def _resample(data, factors):
    """The file with the first component's sampling byte replaced (the header alone: the parser reads no entropy-coded byte)."""
    at = data.index(b"\xff\xc0")
    return data[:at + 11] + bytes([factors]) + data[at + 12:]


def _without_segment(data, marker):
    at = data.index(bytes([0xFF, marker]))
    length = struct.unpack(">H", data[at + 2:at + 4])[0]
    return data[:at] + data[at + 2 + length:]


def test_parse_jpeg_reports_malformed_headers():
    data = model.fixtures()["noise37x51_420"][0]
    info = image_io.parse_jpeg(data)
    for cut in (1, 3, 20, 100, info.segment_offset - 5, info.segment_offset):
        with pytest.raises(ValueError) as e:
            image_io.parse_jpeg(data[:cut])
        assert not isinstance(e.value, image_io.UnsupportedJpeg), cut
    at = data.index(b"\xff\xdb")
    with pytest.raises(ValueError, match="length past the end"):
        image_io.parse_jpeg(data[:at + 2] + b"\xff\xff" + data[at + 4:])
    with pytest.raises(ValueError, match="missing table"):
        image_io.parse_jpeg(_without_segment(_without_segment(data, 0xDB), 0xDB))
    with pytest.raises(ValueError, match="selector without its table"):
        image_io.parse_jpeg(_without_segment(data, 0xDB))            # (Pillow writes one DQT per table: the second stays)
    sof = data.index(b"\xff\xc0")
    with pytest.raises(ValueError, match="zero size"):
        image_io.parse_jpeg(data[:sof + 5] + b"\0\0" + data[sof + 7:])
    with pytest.raises(ValueError, match="no SOI"):
        image_io.parse_jpeg(b"\x89PNG\r\n\x1a\n" + bytes(16))


def test_the_plan_refuses_what_the_kernels_do_not_take():
    info = image_io.parse_jpeg(model.fixtures()["noise8x8_420"][0])
    quant, have_q, bits, vals, have_h = info.plan_tables()
    assert len(ops.jpeg_decode_plan(info.plan_fields(1024), quant, have_q, bits, vals, have_h)) == ops.jpeg_decode_plan_bytes()
    for bad_bits in (48, 0, 1000, 1 << 21):
        with pytest.raises(ValueError, match="subseq_bits"):
            ops.jpeg_decode_plan(info.plan_fields(bad_bits), quant, have_q, bits, vals, have_h)
    with pytest.raises(ValueError, match="selector without its table"):
        ops.jpeg_decode_plan(info.plan_fields(1024), quant, have_q & ~2, bits, vals, have_h)
    full = bytearray(bits)
    full[0:16] = bytes([2] + [0] * 15)                                # two codes of one bit: the second is all ones
    with pytest.raises(ValueError, match="canonical code"):
        ops.jpeg_decode_plan(info.plan_fields(1024), quant, have_q, bytes(full), vals, have_h)
    fields = info.plan_fields(1024)
    fields[3], fields[4] = 1, 2                                       # 4:4:0
    with pytest.raises(ValueError, match="1x1, 2x1 or 2x2"):
        ops.jpeg_decode_plan(fields, quant, have_q, bits, vals, have_h)


def test_bad_arguments_return_minus_one_without_a_gpu():
    from vdpp_amd import hip

    lib = hip.load()
    assert lib.sp_jpeg_decode_plan(None, None, 0, None, None, 0, None) == -1
    assert b"null" in lib.sp_last_error()
    assert lib.sp_jpeg_decode_ws_bytes(None) == 0 and lib.sp_jpeg_decode_coef_bytes(None) == 0
    assert lib.sp_jpeg_decode_split(None, None, None, None, 0, None) == -1
    assert lib.sp_jpeg_decode_sync(None, None, None, 0, 0, 1, None) == -1
    assert lib.sp_jpeg_decode_coefficients(None, None, None, 0, 0, None, None) == -1
    assert lib.sp_jpeg_decode_pixels(None, None, None, 0, None, None, None) == -1
    import ctypes

    junk = ctypes.create_string_buffer(lib.sp_jpeg_decode_plan_bytes())
    assert lib.sp_jpeg_decode_ws_bytes(ctypes.addressof(junk)) == 0
    assert lib.sp_jpeg_decode_split(ctypes.addressof(junk), 16, 16, 16, 1 << 20, None) == -1
    assert b"sp_jpeg_decode_plan" in lib.sp_last_error()


# ------------------------------------------------------------------------------------------------ the model
def _header(height, width, quality, restart_mcus):
    """SOI .. SOS around a segment of jpeg_model.entropy_segment: its tables, 4:2:0, written here from jpeg_model alone."""
    seg = lambda m, body: struct.pack(">BBH", 0xFF, m, len(body) + 2) + body                      # noqa: E731
    out = [b"\xff\xd8"]
    for tq, table in enumerate(jpeg_model.quant_tables(quality)):
        out.append(seg(0xDB, bytes([tq]) + bytes(int(v) for v in table[jpeg_model.ZIGZAG])))
    out.append(seg(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for spec, tc_th in zip(jpeg_model.HUFFMAN_SPECS, (0x00, 0x01, 0x10, 0x11)):
        out.append(seg(0xC4, bytes([tc_th]) + bytes(spec[0]) + bytes(spec[1])))
    out.append(seg(0xDD, struct.pack(">H", restart_mcus)))
    out.append(seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


@pytest.mark.parametrize("kind,h,w,quality,restart", [("noise", 37, 51, 90, 1), ("noise", 48, 64, 100, 4), ("scene", 40, 72, 75, 15),
                                                      ("noise", 17, 16, 5, 3)])
def test_model_decodes_the_encoder_models_segment_exactly(kind, h, w, quality, restart):
    frames = (jpeg_model.noise_frames if kind == "noise" else jpeg_model.scene_frames)(1, h, w, 21)
    coef = jpeg_model.coefficients(frames, quality)[0][0]
    segment, _ = jpeg_model.entropy_segment(coef, restart)
    data = _header(h, w, quality, restart) + segment + b"\xff\xd9"
    assert np.array_equal(model.decode_serial(data), coef)
    got, passes = model.emulate_passes(data, 256)
    assert np.array_equal(got, coef) and passes >= 2
    info = image_io.parse_jpeg(data)                                   # and the package's parser reads that header too
    assert (info.width, info.height, info.hs, info.vs, info.restart_interval) == (w, h, 2, 2, restart)


@pytest.mark.parametrize("name", NAMES)
def test_pass_scheme_equals_the_serial_decode(name):
    data, subseq_bits = model.fixtures()[name]
    coef, passes, _ = model.expected(name)
    assert np.array_equal(coef, model.decode_serial(data))
    stream = model.Stream(data)
    longest = max(-(-8 * (b - a) // subseq_bits) for a, b in zip(stream.bounds, stream.bounds[1:]))
    assert 2 <= passes <= longest + 1, "the count of passes is bounded by the subsequences of the longest interval"


def _parity_text():
    lines = ["Model (tests/jpeg_decode_model.py) against Pillow's decode of the same file, on the CPU, and the count of",
             "synchronisation passes of the model's emulation (the pass that finds nothing changed included).",
             "Written by tests/test_jpeg_decode_cpu.py with JPEG_DECODE_WRITE_PARITY=1; the test fails when it is stale.", "",
             f"{'fixture':<30}{'bytes':>7}{'subseq_bits':>12}{'lanes':>7}{'passes':>7}{'max|diff|':>10}{'mean|diff|':>11}{'equal':>8}"]
    worst, most = 0, 0
    for name in NAMES:
        data, subseq_bits = model.fixtures()[name]
        _, passes, px = model.expected(name)
        d = np.abs(px.astype(np.int64) - model.pillow_pixels(data).astype(np.int64))
        stream = model.Stream(data)
        lanes = sum(-(-8 * (b - a) // subseq_bits) for a, b in zip(stream.bounds, stream.bounds[1:]))
        lines.append(f"{name:<30}{len(data):>7}{subseq_bits:>12}{lanes:>7}{passes:>7}{int(d.max()):>10}{d.mean():>11.4f}{(d == 0).mean():>8.4f}")
        worst = max(worst, int(d.max()))
        if subseq_bits == 1024:
            most = max(most, passes)
    lines += ["", f"largest max|diff|: {worst} (the bound is 4; 0 means the model reproduces libjpeg's integer arithmetic)",
              f"largest count of passes at the default subseq_bits = 1024: {most}; sync_passes K = {most} + 2 = {most + 2}",
              "(the noise pictures at quality 90 and 100 are the worst case: their blocks hold no end-of-block code, so a lane",
              "that starts inside a block finds the true position in the block late; the 144 x 256 scene takes 6 and 9 passes)", ""]
    return "\n".join(lines), worst, most


def test_model_pixels_against_pillow_and_the_parity_file():
    text, worst, most = _parity_text()
    assert worst <= 4
    assert image_io.JPEG_SYNC_PASSES == most + 2, "K is the largest count of passes seen plus 2"
    if os.environ.get("JPEG_DECODE_WRITE_PARITY") == "1":
        with open(PARITY, "w") as fh:
            fh.write(text)
    with open(PARITY) as fh:
        assert fh.read() == text, "profiles/jpeg_decode_parity.txt is stale: run this test with JPEG_DECODE_WRITE_PARITY=1"


def test_upsampling_rounding_on_flat_luma_and_chroma_ramps():
    """Odd sizes, constant luminance, chrominance ramps: every difference to Pillow would be the filter's or the edge rule's."""
    for h, w in ((9, 13), (15, 7), (33, 35), (2, 3), (5, 4)):
        y, x = np.mgrid[0:h, 0:w]
        ycc = np.stack([np.full((h, w), 128), 40 + (170 * x) // max(w - 1, 1), 230 - (190 * y) // max(h - 1, 1)], axis=2).astype(np.uint8)
        from PIL import Image

        rgb = np.asarray(Image.fromarray(ycc, "YCbCr").convert("RGB"))
        for sub in (1, 2):
            data = _pillow_jpeg(rgb, quality=95, subsampling=sub)
            assert np.array_equal(model.pixels(data), model.pillow_pixels(data)), (h, w, sub)


# ------------------------------------------------------------------------------------------------ sanitizer run of the core
def _job(data, subseq_bits):
    info = image_io.parse_jpeg(data)
    quant, have_q, bits, vals, have_h = info.plan_tables()
    return (struct.pack("<19i", *info.plan_fields(subseq_bits), have_q, have_h) + quant + bits + vals
            + data[info.segment_offset:info.segment_offset + info.segment_length])


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "jpeg_decode_hostcheck")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "video-diffusion-pipeline-parallel_amd", "csrc"),
           os.path.join(ROOT, "tools", "jpeg_decode_hostcheck.cpp"), "-o", exe]
    # the runtimes inside the program where the compiler can (gcc links them as shared libraries otherwise), so that the
    # program runs the same under any environment
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    return exe


def _run(exe, tmp_path, jobs):
    """jobs: name -> job bytes.  -> name -> (status of 8 ints, rest of the output); one process, which must end clean."""
    args = []
    for i, (name, job) in enumerate(jobs.items()):
        with open(tmp_path / f"{i}.job", "wb") as fh:
            fh.write(job)
        args += [str(tmp_path / f"{i}.job"), str(tmp_path / f"{i}.out")]
    done = subprocess.run([exe] + args, capture_output=True, text=True)
    assert done.returncode == 0, f"exit status {done.returncode}:\n{done.stderr[-4000:]}"
    out = {}
    for i, name in enumerate(jobs):
        with open(tmp_path / f"{i}.out", "rb") as fh:
            blob = fh.read()
        out[name] = (struct.unpack("<8i", blob[:32]), blob[32:])
    return out


def test_core_under_the_sanitizers_reproduces_the_model(hostcheck, tmp_path):
    results = _run(hostcheck, tmp_path, {name: _job(*model.fixtures()[name]) for name in NAMES})
    for name in NAMES:
        status, rest = results[name]
        coef, passes, px = model.expected(name)
        assert status[0] == 0 and status[1] == 1 and status[7] == 1, (name, status)
        assert status[2] == passes, (name, status)
        assert np.array_equal(np.frombuffer(rest[:coef.size * 2], np.int16).reshape(coef.shape), coef), name
        assert np.array_equal(np.frombuffer(rest[coef.size * 2:], np.uint8).reshape(px.shape), px), name


def test_core_under_the_sanitizers_on_damaged_streams(hostcheck, tmp_path):
    rng = np.random.default_rng(20240607)
    jobs, refused = {}, 0

    def add(name, data, subseq_bits):
        nonlocal refused
        try:
            jobs[name] = _job(data, subseq_bits)
        except ValueError:
            refused += 1                                              # the header itself is damaged: the parser's business

    for base in ("noise37x51_420_rst5", "noise48x64_q90_444"):
        data, subseq_bits = model.fixtures()[base]
        info = image_io.parse_jpeg(data)
        lo, hi = info.segment_offset, info.segment_offset + info.segment_length
        for cut in np.linspace(lo - 40, len(data) - 1, 12).astype(int):
            add(f"{base}/cut{cut}", data[:cut], subseq_bits)
        for i in range(100):
            at, bit = int(rng.integers(lo, hi)), int(rng.integers(0, 8))
            add(f"{base}/flip{i}", data[:at] + bytes([data[at] ^ (1 << bit)]) + data[at + 1:], 256 if i % 2 else subseq_bits)
    data, subseq_bits = model.fixtures()["noise37x51_420_rst1"]
    first, second = data.index(b"\xff\xd0"), data.index(b"\xff\xd1")
    add("removed", data[:first] + data[first + 2:], subseq_bits)
    add("swapped", data[:first + 1] + b"\xd1" + data[first + 2:second + 1] + b"\xd0" + data[second + 2:], subseq_bits)
    assert len(jobs) >= 200 and refused <= 8
    results = _run(hostcheck, tmp_path, jobs)
    for name, (status, rest) in results.items():
        info_fields = struct.unpack("<19i", jobs[name][:76])
        w, h, ncomp, hs, vs = info_fields[:5]
        blocks = -(-w // (8 * hs)) * -(-h // (8 * vs)) * (1 if ncomp == 1 else hs * vs + 2)
        assert status[0] != 0 or (status[7] == 1 and len(rest) == blocks * 128 + h * w * 3), (name, status)
    assert results["removed"][0][0] & 4 and results["swapped"][0][0] & 2
    assert sum(1 for s, _ in results.values() if s[0]) >= 50, "most damage must be noticed"
