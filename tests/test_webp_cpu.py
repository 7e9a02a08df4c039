"""Lossless / animated WebP out, the parts that need no GPU: tests/webp_model.py (the independent statement of the transforms
and of the strip-parallel VP8L stream) through webp_file / write_webp and back through Pillow's libwebp decoder, which is the
judge of the model; the model's file sizes against the PNG model's; the bound; the host routes of save_frames."""

import functools
import io
import warnings

import numpy as np
import pytest

from tests import png_model as pm
from tests import webp_model as wm

SHAPES = [(1, 1, 1), (1, 16, 16), (3, 48, 80), (2, 50, 37), (1, 144, 256)]
KINDS = ("noise", "scene", "correlated")
PARAMS = ((3, 4), (2, 0), (4, 2))               # (pred_bits, group_bits): the defaults; one group; strips of 4 rows


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
def encoded_of(shape, kind, i, pred_bits, group_bits):
    return wm.encode_frame(frames_of(shape, kind)[i], pred_bits, group_bits)


def _open(data):
    """-> (n_frames, size, info of the first frame, RGB frames) with every Pillow warning an error."""
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(data)) as im:
            frames = []
            for i in range(getattr(im, "n_frames", 1)):
                im.seek(i)
                frames.append(np.asarray(im.convert("RGB")))
            return getattr(im, "n_frames", 1), im.size, dict(im.info), frames        # (a frame's duration is known once it is read)


def test_pillow_decodes_webp():
    from PIL import features
    assert features.check("webp"), "Pillow without libwebp cannot judge the model"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_stills_and_animations_decode_in_pillow_to_the_input(shape):
    from vdpp_amd.models.image_io import webp_file, write_webp
    n, h, w = shape
    for kind in KINDS:
        frames = frames_of(shape, kind)
        for pred_bits, group_bits in PARAMS:
            streams = []
            for i in range(n):
                stream, rec = encoded_of(shape, kind, i, pred_bits, group_bits)
                assert stream[0] == 0x2F and len(stream) <= wm.stream_bound(h, w, pred_bits, group_bits)
                assert len(stream) == -(-rec["bits"] // 8)
                assert len(rec["strips"]) == (-(-h // (1 << group_bits)) if group_bits else 1)
                assert rec["residual"][:, :, 3].max() == 0 and int(rec["modes"].max()) <= 13
                if h * w <= 2000:
                    assert np.array_equal(wm.untransform(rec["flag"], rec["modes"], rec["residual"], pred_bits), frames[i])
                data = webp_file(stream)
                assert data == wm.webp_file(stream)
                assert [k for k, _ in wm.walk_webp(data)] == [b"VP8L"]
                count, size, _, pictures = _open(data)
                assert count == 1 and size == (w, h) and np.array_equal(pictures[0], frames[i]), f"{kind} {pred_bits} {group_bits} frame {i}"
                streams.append(stream)
            movie = write_webp(None, streams, w, h, 7)
            assert movie == wm.webp_animation(streams, w, h, 7)
            chunks = wm.walk_webp(movie)
            assert [k for k, _ in chunks] == [b"VP8X", b"ANIM"] + [b"ANMF"] * n
            assert chunks[0][1] == bytes([2, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
            assert chunks[1][1] == bytes(6)
            for (_, (head, inner)), stream in zip(chunks[2:], streams):
                assert head == bytes(6) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little") + (143).to_bytes(3, "little") + b"\x02"
                assert inner == [(b"VP8L", stream)]
            count, size, info, pictures = _open(movie)
            assert count == n and size == (w, h) and all(np.array_equal(p, f) for p, f in zip(pictures, frames))
            if n > 1:                                                      # (Pillow opens a one-frame animation as a still)
                assert info.get("duration") == 143 and info.get("loop") == 0


def test_write_webp_of_the_models_streams(tmp_path):
    from vdpp_amd.models.image_io import write_webp
    shape = (3, 48, 80)
    streams = [encoded_of(shape, "scene", i, 3, 4)[0] for i in range(3)]
    assert any(len(s) & 1 for s in streams) or len(encoded_of(shape, "noise", 0, 3, 4)[0]) & 1, "an odd payload must be among the cases"
    path = tmp_path / "a.webp"
    data = write_webp(str(path), streams, 80, 48, 7)
    assert path.read_bytes() == data == wm.webp_animation(streams, 80, 48, 7) and len(data) % 2 == 0
    count, size, info, pictures = _open(data)
    assert count == 3 and size == (80, 48) and info.get("loop") == 0 and info.get("duration") == 143
    assert _open(write_webp(None, streams, 80, 48, 12.5))[2]["duration"] == 80
    with pytest.raises(ValueError):
        write_webp(None, [], 80, 48, 7)
    for fps in (0, -1, None, "7", 1e-5):
        with pytest.raises(ValueError):
            write_webp(None, streams, 80, 48, fps)
    for w, h in ((0, 48), (80, 16385)):
        with pytest.raises(ValueError):
            write_webp(None, streams, w, h, 7)


def test_sizes_at_the_default_parameters():
    """Conditions, not measurements.  Observed: the scene frame 76,850 bytes against 78,288 of the PNG model at strips of 16
    rows; the correlated frame 53,332 against 78,061 (0.683)."""
    from vdpp_amd.models.image_io import WEBP_GROUP_BITS, WEBP_PRED_BITS
    scene = pm.scene_frames(1, 144, 256, seed=5)[0]
    corr = wm.correlated_frame(144, 256, seed=5)
    assert np.array_equal(corr[:, :, 1], scene[:, :, 1])
    assert wm.subtract_green_costs(scene) == (1115083, 799151) and wm.subtract_green_costs(corr) == (126902, 780660)
    sizes = {}
    for name, frame in (("scene", scene), ("correlated", corr)):
        png = len(pm.png_file(144, 256, pm.deflate_stream(pm.filter_frame(frame), 16)[0]))
        stream, rec = wm.encode_frame(frame, WEBP_PRED_BITS, WEBP_GROUP_BITS)
        sizes[name] = (len(wm.webp_file(stream)), png, rec["flag"])
        print(f"{name}: {sizes[name][0]} bytes of WebP, {png} of PNG, subtract green {rec['flag']}")
        assert np.array_equal(_open(wm.webp_file(stream))[3][0], frame)
    assert sizes["scene"][2] == 0 and sizes["correlated"][2] == 1
    assert sizes["scene"][0] <= sizes["scene"][1]
    assert sizes["correlated"][0] <= 0.75 * sizes["correlated"][1]


def test_coder_corners_exist_in_the_model():
    fib = wm.fibonacci_values()
    counts = [int(np.count_nonzero(fib == v)) for v in range(256)]
    assert max(pm.huffman_depths(counts)) > 15
    lengths, halvings = pm.huffman_lengths(counts, 15)
    assert halvings >= 1 and max(lengths) <= 15 and sum(2.0 ** -n for n in lengths if n) == 1.0, "a normal code is complete"
    bits = pm._Bits()
    assert wm.write_code(bits, [0] * 40)[2]["simple"] and bits.n == 4
    bits = pm._Bits()
    assert wm.write_code(bits, [0] * 255 + [9])[2]["simple"] and bits.n == 11
    bits = pm._Bits()
    lengths, _, rec = wm.write_code(bits, [0] * 256 + [5] + [0] * 23)      # one length symbol alone: never a one-leaf code
    assert not rec["simple"] and lengths[0] == 1 and lengths[256] == 1 and sum(lengths) == 2
    assert wm.tokens([7] * 3) == [("lit", 7)] * 3 and wm.tokens([7] * 4) == [("lit", 7), ("copy", 3)]
    assert wm.tokens([7] * 4099) == [("lit", 7), ("copy", 4096), ("lit", 7), ("lit", 7)]
    assert wm.prefix_symbol(1) == (0, 0, 0) and wm.prefix_symbol(4096) == (23, 10, 1023) and wm.prefix_symbol(2) == (1, 0, 0)
    modes = wm.transform(wm.every_mode_frame(2), 2)[1]
    assert set(range(1, 14)) <= {int(m) for m in modes.reshape(-1)}
    # predictor 13 truncates toward zero: floor would give another residual where a - TL is odd and negative
    assert int(wm._predict(13, [10] * 3, [11] * 3, [15] * 3, [0] * 3)[0]) == 10 - 2


def test_stream_bound_is_what_the_header_derives_and_holds_on_noise():
    from vdpp_amd.hip import ops
    assert wm.GROUP_HEADER_MAX == 11285 and wm.SUB_HEADER_MAX == 7649
    for n, h, w in SHAPES:
        for pred_bits, group_bits in PARAMS:
            bound = wm.stream_bound(h, w, pred_bits, group_bits)
            assert ops.webp_stream_bytes(h, w, pred_bits, group_bits) == bound
            assert ops.webp_ws_bytes(2, h, w, pred_bits, group_bits) > 0
            assert len(encoded_of((n, h, w), "noise", 0, pred_bits, group_bits)[0]) <= bound
    for bad in ((0, 4, 3, 4), (4, 0, 3, 4), (16385, 1, 3, 4), (1, 16385, 3, 4), (8192, 4096, 3, 4), (4, 4, 1, 4), (4, 4, 10, 4), (4, 4, 3, 1),
                (4, 4, 3, 10), (4, 4, 3, -1)):
        assert ops.webp_stream_bytes(*bad) == 0 and ops.webp_ws_bytes(1, *bad) == 0, bad
    assert ops.webp_ws_bytes(0, 8, 8, 3, 4) == 0 and ops.webp_stream_bytes(16384, 1024, 9, 9) > 0


def test_save_frames_host_routes(tmp_path):
    import torch

    from vdpp_amd.models.image_io import save_frames
    frames = pm.scene_frames(3, 20, 28, seed=2)
    for name, given in (("a.webp", frames), ("t.webp", torch.from_numpy(frames))):
        assert save_frames(given, str(tmp_path / name), fps=7) == [str(tmp_path / name)]
        count, size, info, pictures = _open((tmp_path / name).read_bytes())
        assert count == 3 and size == (28, 20) and all(np.array_equal(p, f) for p, f in zip(pictures, frames))
        assert info.get("duration") == 143 and info.get("loop") == 0
    names = save_frames(frames, str(tmp_path / "f_%03d.webp"))
    assert names == [str(tmp_path / f"f_{k:03d}.webp") for k in range(3)]
    for name, f in zip(names, frames):
        count, size, _, pictures = _open(open(name, "rb").read())
        assert count == 1 and size == (28, 20) and np.array_equal(pictures[0], f)
    with pytest.raises(ValueError):
        save_frames(frames.astype(np.float32), str(tmp_path / "z.webp"))
    with pytest.raises(ValueError):
        save_frames(frames, str(tmp_path / "z.webp"), fps=0)
    assert not (tmp_path / "z.webp").exists()
    with pytest.raises(ValueError, match="imageio / ffmpeg") as refused:
        save_frames(frames, str(tmp_path / "x.mp4"))
    assert ".webp" in str(refused.value)
    with pytest.raises(ValueError, match="unknown output format") as refused:
        save_frames(frames, str(tmp_path / "x.bmp"))
    assert ".webp" in str(refused.value)
