"""The frame interpolator's numpy statement (tests/interp_model.py) held to its own properties, the planted mistakes it
must tell apart, and the host side of ``save_frames(..., interpolate=)``.  No GPU.

Properties: a static pair comes back exactly; a crop of a larger picture that moves by 2u between A and B gives the crop
moved by u EXACTLY at every pixel farther than 2 max(|uy|, |ux|) + 8 from the border (a pixel's four blocks then search
windows that, displaced by +-u, stay inside both frames, so the true vector costs 0 + lam |u| and on noise nothing else
comes near); on a scene of two objects over a static background the midpoint is at least 3 dB closer to the true middle
frame than the rounded average of A and B is."""

import functools
import os

import numpy as np
import pytest

from tests import interp_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITY = os.path.join(ROOT, "profiles", "interp_quality.txt")


@functools.lru_cache(maxsize=None)
def picture(kind: str, h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if kind == "white" else im.smoothed_noise(rng, h, w)
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("kind", ["white", "smooth"])
def test_static_pair_is_exact(kind):
    f = picture(kind, 48, 64, 3)
    out, vectors, raw = im.interpolate_round(np.stack([f, f, f]), 16, 4)
    assert out.shape == (5, 48, 64, 3)
    assert all(np.array_equal(o, f) for o in out)
    assert not vectors.any() and not raw.any()


def _check_translation(kind, h, w, u, R):
    m = 2 * max(abs(u[0]), abs(u[1]))
    pic = picture(kind, h + 2 * m + 8, w + 2 * m + 8, 7)
    pair = im.moving_crop(pic, h, w, u)
    out, vectors, _ = im.interpolate_round(pair, R, 4)
    assert np.array_equal(out[0], pair[0]) and np.array_equal(out[2], pair[1])
    truth = im.crop_at(pic, h, w, u)
    margin = m + 8
    assert h > 2 * margin and w > 2 * margin, "the case must leave an interior"
    wrong = (out[1] != truth).any(axis=-1)
    ys, xs = np.nonzero(wrong)
    depth = np.minimum.reduce([ys, h - 1 - ys, xs, w - 1 - xs]).max() if ys.size else -1
    print(f"{kind} u={u} R={R} {h}x{w}: deepest wrong pixel {depth} from the border, exact beyond {margin}")
    assert not wrong[margin:h - margin, margin:w - margin].any(), f"u={u}: wrong pixels as deep as {depth}, beyond the margin {margin}"
    inner = vectors[0][(margin + 7) // 8 + 1: (h - margin) // 8 - 1, (margin + 7) // 8 + 1: (w - margin) // 8 - 1]
    assert (inner == np.array(u, np.int16)).all()


@pytest.mark.parametrize("kind", ["white", "smooth"])
@pytest.mark.parametrize("u", [(1, 0), (5, -3), (-7, 11), (16, -16), (-16, 9), (13, 16)])
def test_translation_is_exact_beyond_the_margin(kind, u):
    _check_translation(kind, 96, 128, u, 16)


def test_translation_at_the_largest_range():
    _check_translation("smooth", 128, 144, (24, -24), 24)        # |u| = R = 24: margin 56, an interior of 16 x 32


def _quality_rows():
    rows = []
    for seed in (0, 1):
        a, mid, b = im.two_object_scene(np.random.default_rng(seed))
        base = im.psnr(im.rounded_average(a, b), mid)
        for R in (8, 16):
            got = im.psnr(im.interpolate_round(np.stack([a, b]), R, 4)[0][1], mid)
            rows.append((seed, R, got, base))
    return rows


def test_two_object_scene_beats_the_rounded_average_by_3_db():
    rows = _quality_rows()
    lines = ["PSNR (dB) of the interpolated midpoint against the true middle frame, and of the rounded average of A and B: the",
             "numpy statement (tests/interp_model.py; the kernels equal it bit for bit) on a 128x192 scene of a static",
             "smoothed-noise background, a 48x48 patch that moves (8, 12) from A to B and a 40x56 patch that moves (-6, 4).",
             "lam = 4.  Written by tests/test_interp_cpu.py with INTERP_WRITE_QUALITY=1; the test fails when it is stale.",
             "Not a statement about a learned interpolator's quality, nor about occlusions beyond the blend.", "",
             f"{'seed':>5}{'R':>4}{'midpoint':>10}{'average':>9}{'gain':>7}"]
    for seed, R, got, base in rows:
        lines.append(f"{seed:>5}{R:>4}{got:>10.2f}{base:>9.2f}{got - base:>7.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    for seed, R, got, base in rows:
        assert got >= base + 3.0, f"seed {seed}, R = {R}: {got:.2f} dB against the average's {base:.2f} dB"
    if os.environ.get("INTERP_WRITE_QUALITY") == "1":
        with open(QUALITY, "w") as fh:
            fh.write(text)
    with open(QUALITY) as fh:
        assert fh.read() == text, "profiles/interp_quality.txt is stale: run this test with INTERP_WRITE_QUALITY=1"


# ------------------------------------------------------------------------------------------------ planted mistakes
@functools.lru_cache(maxsize=None)
def mutant_inputs():
    """(name, frames, R, lam): small enough that all eleven mutants run in a second or two."""
    rng = np.random.default_rng(11)
    h, w, R = 32, 40, 3
    noise = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    moved = im.moving_crop(picture("smooth", h + 16, w + 16, 5), h, w, (2, -1))
    flat = np.full((2, h, w, 3), 90, np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    # depends on x + y only: every v with vy + vx = 0 costs the same, and the two index orders rank those differently
    diagonal = np.repeat(((37 * (x + y)) % 251).astype(np.uint8)[None, :, :, None], 3, axis=3).repeat(2, axis=0)
    dark = (noise >> 5) + np.array([1, 0, 2], np.uint8)          # low levels: the luma's rounding term decides
    return (("noise", noise, R, 2), ("moved", moved, R, 2), ("flat", flat, R, 2), ("flat lam 0", flat, R, 0),
            ("diagonal lam 0", diagonal, R, 0), ("dark", dark, R, 2))


@functools.lru_cache(maxsize=None)
def statement(i: int):
    _, frames, R, lam = mutant_inputs()[i]
    return im.interpolate_round(frames, R, lam)


@pytest.mark.parametrize("mutant", im.MUTANTS)
def test_planted_mistake_changes_a_vector_or_a_byte(mutant):
    seen = []
    for i, (name, frames, R, lam) in enumerate(mutant_inputs()):
        got = im.interpolate_round(frames, R, lam, mutant=mutant)
        if any(not np.array_equal(g, s) for g, s in zip(got, statement(i))):
            seen.append(name)
    print(f"{mutant}: seen on {seen}")
    assert seen, f"the planted mistake '{mutant}' changes nothing on the test inputs"


def test_model_refuses_what_the_kernels_refuse():
    ok = np.zeros((2, 16, 16, 3), np.uint8)
    for bad in (ok[:1], np.zeros((2, 12, 16, 3), np.uint8), np.zeros((2, 16, 20, 3), np.uint8), ok.astype(np.int16), ok[..., :2]):
        with pytest.raises(ValueError):
            im.interpolate(bad)
    for kw in ({"R": 0}, {"R": 25}, {"lam": -1}, {"lam": 256}, {"factor": 3}):
        with pytest.raises(ValueError):
            im.interpolate(ok, **kw)
    assert im.interpolate(ok, factor=1) is not None and im.interpolate(ok, factor=4).shape == (5, 16, 16, 3)


# ------------------------------------------------------------------------------------------------ save_frames, host side
def test_save_frames_interpolate_argument_on_the_host(tmp_path):
    import torch
    from vdpp_amd.models.image_io import save_frames
    frames = np.random.default_rng(2).integers(0, 256, (3, 16, 24, 3), dtype=np.uint8)
    for name in ("a.gif", "a.apng", "a.npy", "f_%03d.png"):
        plain = save_frames(frames, str(tmp_path / name), fps=6)
        before = [open(p, "rb").read() for p in plain]
        again = save_frames(frames, str(tmp_path / ("b" + name)), fps=6, interpolate=1)
        assert [open(p, "rb").read() for p in again] == before, f"{name}: interpolate=1 must write what no argument writes"
    for given in (frames, torch.from_numpy(frames)):
        for factor in (2, 4):
            with pytest.raises(ValueError, match="device"):
                save_frames(given, str(tmp_path / "c.gif"), fps=6, interpolate=factor)
    for factor in (0, 3, 8, -2, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="interpolate"):
            save_frames(frames, str(tmp_path / "c.gif"), fps=6, interpolate=factor)
    assert not (tmp_path / "c.gif").exists()


def test_generate_takes_the_interpolation_options():
    from vdpp_amd.modes.generate import parse_args
    base = ["--input-image", "x.png", "--output", "y.gif", "--random-init"]
    a = parse_args(base)
    assert (a.interpolate, a.interp_range, a.interp_penalty) == (1, 16, 4)
    a = parse_args(base + ["--interpolate", "4", "--interp-range", "8", "--interp-penalty", "0"])
    assert (a.interpolate, a.interp_range, a.interp_penalty) == (4, 8, 0)
    for bad in (["--interpolate", "3"], ["--interp-range", "0"], ["--interp-range", "25"], ["--interp-penalty", "256"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
