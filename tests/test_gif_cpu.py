"""Animated GIF out, the parts that need no GPU: tests/gif_model.py (the independent statement of the quantiser and of the
strip-parallel LZW stream) through write_gif and back through Pillow and through the model's own strict decoder, the file
against a strict block walker, the refusals of write_gif and of the size functions, and the unchanged host route."""

import io
import warnings

import numpy as np
import pytest

from tests import gif_model as gm

Image = pytest.importorskip("PIL.Image")

SHAPES = [(2, 16, 16), (2, 50, 37), (1, 64, 128), (1, 96, 256)]


def _open(data):
    """-> (n_frames, size, info of the first frame, RGB frames) with every Pillow warning an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(data)) as im:
            info, frames = dict(im.info), []
            for i in range(im.n_frames):
                im.seek(i)
                frames.append(np.asarray(im.convert("RGB")))
            return im.n_frames, im.size, info, frames


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_through_write_gif_opens_in_pillow(shape):
    from vdpp_amd.models.image_io import write_gif
    n, h, w = shape
    for kind in (gm.noise_frames, gm.scene_frames):
        frames = kind(n, h, w, seed=h + w)
        palettes, indices, used = gm.quantise_frames(frames)
        assert indices.shape == (n, h, w) and all(int(indices[i].max()) < used[i] for i in range(n))
        for strip_rows in (1, 3, 16, h):
            datas = [gm.lzw_image_data(indices[i], strip_rows)[0] for i in range(n)]
            data = write_gif(None, palettes, datas, w, h, 7)
            assert data == gm.gif_file(palettes, datas, w, h, 7)
            count, size, info, pictures = _open(data)
            assert count == n and size == (w, h)
            assert info.get("loop") == 0 and info.get("duration") == 140
            walked = gm.walk_gif(data)
            assert walked["size"] == (w, h) and walked["loop"] == 0 and len(walked["frames"]) == n
            for i in range(n):
                assert np.array_equal(pictures[i], palettes[i][indices[i]]), f"{kind.__name__} strip rows {strip_rows} frame {i}"
                fr = walked["frames"][i]
                assert fr["delay"] == 14 and fr["rect"] == (0, 0, w, h) and fr["min_code"] == 8 and fr["disposal"] == 0
                assert np.array_equal(fr["palette"], palettes[i])
                assert b"\x08" + gm.sub_blocks(fr["data"]) == datas[i]
                assert gm.lzw_decode(fr["data"]) == indices[i].reshape(-1).tolist()


def test_model_quantiser_keeps_few_colours_and_beats_pillows_median_cut():
    rng = np.random.default_rng(5)
    colours = np.stack([rng.permutation(32)[:30] * 8 + rng.integers(0, 8, 30) for _ in range(3)], axis=1)   # 30 distinct bins
    frame = colours[rng.integers(0, 30, (24, 40))].astype(np.uint8)
    palette, indices, used = gm.quantise(frame)
    assert used == len(np.unique(frame.reshape(-1, 3), axis=0)) and np.array_equal(palette[indices], frame)
    assert not palette[used:].any()
    palette, indices, used = gm.quantise(np.full((5, 7, 3), 200, dtype=np.uint8))
    assert used == 1 and not indices.any() and palette[0].tolist() == [200, 200, 200]
    for kind in (gm.noise_frames, gm.scene_frames):
        frame = kind(1, 96, 160, seed=3)[0]
        palette, indices, used = gm.quantise(frame)
        assert used == 256
        theirs = np.asarray(Image.fromarray(frame).quantize(256, method=0, dither=Image.Dither.NONE).convert("RGB"))
        ours = gm.psnr(palette[indices], frame)
        print(f"{kind.__name__}: {ours:.3f} dB, Pillow's median cut {gm.psnr(theirs, frame):.3f} dB")
        assert ours >= gm.psnr(theirs, frame) - 0.05


def test_write_gif_file_and_refusals(tmp_path):
    from vdpp_amd.models.image_io import write_gif
    palettes, indices, _ = gm.quantise_frames(gm.scene_frames(2, 8, 12, seed=1))
    datas = [gm.lzw_image_data(i, 16)[0] for i in indices]
    path = tmp_path / "a.gif"
    data = write_gif(str(path), [p.tobytes() for p in palettes], datas, 12, 8, 10)
    assert path.read_bytes() == data and data[:6] == b"GIF89a" and data[-1] == 0x3B
    assert [f["delay"] for f in gm.walk_gif(data)["frames"]] == [10, 10]
    assert gm.walk_gif(write_gif(None, palettes, datas, 12, 8, 1000))["frames"][0]["delay"] == 1     # never 0: players stall
    assert gm.walk_gif(write_gif(None, palettes, datas, 12, 8, 7.5))["frames"][0]["delay"] == 13
    with pytest.raises(ValueError):
        write_gif(None, [], [], 12, 8, 7)
    with pytest.raises(ValueError):
        write_gif(None, palettes, datas[:1], 12, 8, 7)
    for fps in (0, -1, None, "7"):
        with pytest.raises(ValueError):
            write_gif(None, palettes, datas, 12, 8, fps)
    for w, h in ((0, 8), (12, 0), (65536, 8)):
        with pytest.raises(ValueError):
            write_gif(None, palettes, datas, w, h, 7)
    with pytest.raises(ValueError):
        write_gif(None, [palettes[0][:255]] * 2, datas, 12, 8, 7)
    assert not (tmp_path / "b.gif").exists()


def test_host_arrays_still_go_through_pillow(tmp_path):
    """The bytes of the parent commit's route, restated here: Pillow's own writer on the array."""
    import torch

    from vdpp_amd.models.image_io import save_frames
    frames = gm.scene_frames(3, 20, 28, seed=2)
    ims = [Image.fromarray(f) for f in frames]
    want = io.BytesIO()
    ims[0].save(want, format="GIF", save_all=True, append_images=ims[1:], loop=0, duration=1000.0 / 6)
    for name, given in (("a.gif", frames), ("t.gif", torch.from_numpy(frames))):
        assert save_frames(given, str(tmp_path / name), fps=6) == [str(tmp_path / name)]
        assert (tmp_path / name).read_bytes() == want.getvalue()
    with pytest.raises(ValueError):
        save_frames(frames, str(tmp_path / "z.gif"), fps=0)


def test_size_functions_need_no_gpu_and_refuse_bad_arguments():
    from vdpp_amd.hip import ops
    assert ops.gif_stream_bytes(576, 1024, 16) > 0 and ops.gif_ws_bytes(14, 576, 1024, 16) > 0
    assert ops.gif_stream_bytes(4096, 4096, 1) > 0 and ops.gif_stream_bytes(1, 1, 100) == ops.gif_stream_bytes(1, 1, 1)
    for h, w, rows in ((0, 8, 1), (8, 0, 1), (65536, 1, 1), (1, 65536, 1), (4097, 4096, 16), (8, 8, 0), (8, 8, -3), (-1, 8, 1)):
        assert ops.gif_stream_bytes(h, w, rows) == 0, (h, w, rows)
        assert ops.gif_ws_bytes(1, h, w, rows) == 0, (h, w, rows)
    assert ops.gif_ws_bytes(0, 8, 8, 1) == 0 and ops.gif_ws_bytes(-1, 8, 8, 1) == 0
    # the bound as the header derives it: 12 bits per pixel, a CLEAR per 3838 codes, the ends of the strips, a byte per 255
    for h, w, rows in ((576, 1024, 16), (50, 37, 3), (1, 4200, 1), (64, 128, 64)):
        strips = -(-h // rows)
        nbytes = -(-(9 + 12 * h * w + 12 * (h * w // (gm.TABLE_END - gm.FIRST_FREE)) + 12 * strips) // 8)
        assert ops.gif_stream_bytes(h, w, rows) == 1 + nbytes + -(-nbytes // 255) + 1
