"""PNG / APNG out, the parts that need no GPU: tests/png_model.py (the independent statement of the row filter and of the
strip-parallel deflate stream) through zlib, through png_file / write_apng and back through Pillow; the model's file size
against Pillow's default save; the host routes of save_frames."""

import functools
import io
import warnings
import zlib

import numpy as np
import pytest

from tests import png_model as pm

Image = pytest.importorskip("PIL.Image")

SHAPES = [(1, 1, 1), (1, 16, 16), (3, 48, 80), (2, 50, 37), (1, 144, 256)]
KINDS = ("noise", "scene")


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


def _open(data):
    """-> (n_frames, size, info of the first frame, RGB frames) with every Pillow warning an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(data)) as im:
            info, frames = dict(im.info), []
            for i in range(getattr(im, "n_frames", 1)):
                im.seek(i)
                frames.append(np.asarray(im.convert("RGB")))
            return getattr(im, "n_frames", 1), im.size, info, frames


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_stream_inflates_to_the_filtered_bytes_and_the_file_opens_in_pillow(shape):
    from vdpp_amd.models.image_io import png_file
    n, h, w = shape
    for kind in KINDS:
        frames, filtered = frames_of(shape, kind), filtered_of(shape, kind)
        assert filtered.shape == (n, h, 1 + 3 * w) and int(filtered[:, :, 0].max()) <= 4
        for i in range(n):
            assert np.array_equal(pm.unfilter(filtered[i], w), frames[i]) if h * w <= 2000 else True
            for strip_rows in sorted({1, 3, 8, h}):
                stream, strips = pm.deflate_stream(filtered[i], strip_rows)
                assert len(strips) == -(-h // strip_rows)
                assert zlib.decompress(stream) == filtered[i].tobytes(), f"{kind} strip rows {strip_rows} frame {i}"
                assert stream[-4:] == pm.adler32(filtered[i].tobytes()).to_bytes(4, "big")
                assert len(stream) <= pm.stream_bound(h, w, strip_rows)
                data = png_file(h, w, stream)
                assert data == pm.png_file(h, w, stream)
                assert [k for k, _ in pm.walk_png(data)] == [b"IHDR", b"IDAT", b"IEND"]
                count, size, _, pictures = _open(data)
                assert count == 1 and size == (w, h) and np.array_equal(pictures[0], frames[i])
        top = filtered[0][:min(3, h)].reshape(-1).tolist()
        assert pm.tokens(top) == pm.tokens_by_runs(top), "the greedy rule and the per-run rule must give the same tokens"


def test_write_apng_of_the_models_streams_opens_in_pillow(tmp_path):
    from vdpp_amd.models.image_io import write_apng
    shape = (3, 48, 80)
    frames, filtered = frames_of(shape, "scene"), filtered_of(shape, "scene")
    streams = [pm.deflate_stream(f, 8)[0] for f in filtered]
    path = tmp_path / "a.apng"
    data = write_apng(str(path), streams, 80, 48, 7)
    assert path.read_bytes() == data == pm.apng_file(streams, 80, 48, 7)
    kinds = [k for k, _ in pm.walk_png(data)]
    assert kinds == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    count, size, info, pictures = _open(data)
    assert count == 3 and size == (80, 48) and info.get("loop") == 0
    assert abs(info.get("duration") - 1000.0 / 7) < 1e-6
    for i in range(3):
        assert np.array_equal(pictures[i], frames[i])
    assert abs(_open(write_apng(None, streams, 80, 48, 12.5))[2]["duration"] - 80.0) < 1e-6
    with pytest.raises(ValueError):
        write_apng(None, [], 80, 48, 7)
    for fps in (0, -1, None, "7"):
        with pytest.raises(ValueError):
            write_apng(None, streams, 80, 48, fps)
    with pytest.raises(ValueError):
        write_apng(None, streams, 0, 48, 7)


def test_model_file_is_no_larger_than_pillows_default_save():
    """The bound is Pillow itself: its default PNG of the same frame (zlib level 6, its own filter choice)."""
    shape = (1, 144, 256)
    frame, filtered = frames_of(shape, "scene")[0], filtered_of(shape, "scene")[0]
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="PNG")
    for strip_rows in (8, 16):
        ours = len(pm.png_file(144, 256, pm.deflate_stream(filtered, strip_rows)[0]))
        print(f"strip rows {strip_rows}: {ours} bytes, Pillow {len(buf.getvalue())}")
        assert ours <= len(buf.getvalue())


def test_coder_corners_exist_in_the_model():
    row = pm.fibonacci_row()
    counts = [int(np.count_nonzero(row == v)) for v in range(256)] + [1]
    assert max(pm.huffman_depths(counts)) > 15
    stream, strips = pm.deflate_stream(row[None], 1)
    assert strips[0]["halvings"] >= 1 and max(strips[0]["lengths"]) <= 15 and zlib.decompress(stream) == row.tobytes()
    assert pm.huffman_lengths([0, 0, 5, 0], 7)[0] == [1, 0, 1, 0], "one symbol in use: the lowest unused one joins it"
    assert pm.huffman_lengths([0] * 4, 7)[0] == [1, 1, 0, 0]
    types = {int(t) for t in pm.filter_frames(pm.ramps())[:, :, 0].reshape(-1)}
    assert len(types) >= 4, types


def test_save_frames_host_routes(tmp_path):
    import torch

    from vdpp_amd.models.image_io import save_frames
    frames = pm.scene_frames(3, 20, 28, seed=2)
    for name, given in (("a.apng", frames), ("t.apng", torch.from_numpy(frames))):
        assert save_frames(given, str(tmp_path / name), fps=6) == [str(tmp_path / name)]
        count, size, info, pictures = _open((tmp_path / name).read_bytes())
        assert count == 3 and size == (28, 20) and all(np.array_equal(p, f) for p, f in zip(pictures, frames))
        assert abs(info.get("duration") - 1000.0 / 6) < 1e-6
    with pytest.raises(ValueError):
        save_frames(frames, str(tmp_path / "z.apng"), fps=0)
    with pytest.raises(ValueError):
        save_frames(frames, str(tmp_path / "x.png"))
    assert not (tmp_path / "x.png").exists() and not (tmp_path / "z.apng").exists()
    # PNG frames of a host array: Pillow's own bytes, as before
    names = save_frames(frames, str(tmp_path / "f_%03d.png"))
    want = io.BytesIO()
    Image.fromarray(frames[1]).save(want, format="PNG")
    assert len(names) == 3 and open(names[1], "rb").read() == want.getvalue()
    assert len(save_frames(frames, str(tmp_path / "dir"))) == 3 and (tmp_path / "dir" / "002.png").exists()


def test_size_functions_need_no_gpu_and_refuse_bad_arguments():
    from vdpp_amd.hip import ops
    assert ops.png_stream_bytes(4096, 4096, 1) > 0 and ops.png_stream_bytes(1, 1, 100) == ops.png_stream_bytes(1, 1, 1)
    for h, w, rows in ((0, 8, 1), (8, 0, 1), (65536, 1, 1), (1, 65536, 1), (4097, 4096, 16), (8, 8, 0), (8, 8, -3), (-1, 8, 1)):
        assert ops.png_stream_bytes(h, w, rows) == 0, (h, w, rows)
        assert ops.png_ws_bytes(1, h, w, rows) == 0, (h, w, rows)
    assert ops.png_ws_bytes(0, 8, 8, 1) == 0 and ops.png_ws_bytes(-1, 8, 8, 1) == 0
    for h, w, rows in ((576, 1024, 8), (50, 37, 3), (1, 1400, 1), (64, 128, 64), (64, 128, 100)):
        assert ops.png_stream_bytes(h, w, rows) == pm.stream_bound(h, w, rows)
        assert ops.png_ws_bytes(2, h, w, rows) > 0
