"""Large frames as overlapping spatial tiles, without a GPU: the host plan (``models/tile_plan.py``) against the fp64 statement
(``tests/tile_model.py``), the statement against itself and against ``tests/window_model.py``, the planted mistakes against the
kernel bound of ``tests/test_tile_gpu.py`` on that test's own inputs, and the argument errors of the generate mode.

The consistency and planted-mistake tests prove things about the statement, not about product code; they check first that the
statement's tables are the ones ``models/tile_plan.plan`` makes."""

import numpy as np
import pytest

from tests import tile_model as tm
from tests import window_model as wm

# (H, W, th, tw, sy, sx)
PLANS = [(6, 12, 4, 8, 2, 4), (5, 7, 3, 3, 1, 2), (4, 8, 2, 4, 2, 4), (9, 16, 9, 8, 3, 8), (8, 16, 8, 16, 5, 16)]


def _plan(*a, **kw):
    from vdpp_amd.models import tile_plan
    return tile_plan.plan(*a, **kw)


@pytest.mark.parametrize("weights", ["triangle", "uniform"])
@pytest.mark.parametrize("frames", [(1, None, None), (6, 4, 2)], ids=["one-window", "two-windows"])
@pytest.mark.parametrize("geom", PLANS, ids=str)
def test_plan_properties(geom, frames, weights):
    """Over the patches covering any element the product weights sum to 1 within fp32 rounding; the product of the three
    normalised tables is the normalised product profile (separable); coverage is at most ``ceil(t/s)`` per axis; the patch
    order is ``(kf*n_ty + ky)*n_tx + kx``; the tables are those of the fp64 statement."""
    h, w, th, tw, sy, sx = geom
    ft, win, st = frames
    pl = _plan(h, w, (th, tw), (sy, sx), weights, frames_total=ft, window=win, window_stride=st)
    n_ty, n_tx = (h - th) // sy + 1, (w - tw) // sx + 1
    n_win = 1 if win is None else (ft - win) // st + 1
    wf_len = ft if win is None else win
    assert (pl.n_ty, pl.n_tx, pl.frames.n_win, pl.n_patch, pl.tile) == (n_ty, n_tx, n_win, n_win * n_ty * n_tx, (th, tw))
    for table, shape in ((pl.wf, (n_win, wf_len)), (pl.wy, (n_ty, th)), (pl.wx, (n_tx, tw))):
        assert table.dtype == np.float32 and table.shape == shape and (table > 0).all()
    if win is None:
        assert np.array_equal(pl.wf, np.ones((1, ft), dtype=np.float32))
    shape = (1, ft, wf_len, st or ft, h, w, th, tw, sy, sx)
    for (starts, table), mine, axis in zip(tm.plans(shape, weights), (pl.wf, pl.wy, pl.wx), (pl.frames, pl.y, pl.x)):
        assert starts == list(axis.starts) and np.array_equal(table.astype(np.float32), mine)
    patches = pl.patches()
    assert [pl.patch_index(kf, ky, kx) for kf, ky, kx, *_ in patches] == list(range(pl.n_patch))
    assert all((f0, y0, x0) == (pl.frames.starts[kf], pl.y.starts[ky], pl.x.starts[kx]) for kf, ky, kx, f0, y0, x0 in patches)
    # the sum of the fp32 product weights, and the normalised product profile made directly in fp64
    alpha = [wm.profile(wf_len, weights), wm.profile(th, weights), wm.profile(tw, weights)]
    total, raw, count = np.zeros((ft, h, w)), np.zeros((ft, h, w)), np.zeros((ft, h, w), dtype=np.int64)
    for kf, ky, kx, f0, y0, x0 in patches:
        sel = np.s_[f0:f0 + wf_len, y0:y0 + th, x0:x0 + tw]
        prod32 = (pl.wf[kf][:, None, None] * pl.wy[ky][None, :, None]) * pl.wx[kx][None, None, :]
        assert prod32.dtype == np.float32
        total[sel] += prod32.astype(np.float64)
        raw[sel] += alpha[0][:, None, None] * alpha[1][None, :, None] * alpha[2][None, None, :]
        count[sel] += 1
    assert np.abs(total - 1.0).max() <= 8 * 2.0 ** -22, np.abs(total - 1.0).max()
    for kf, ky, kx, f0, y0, x0 in patches:
        sel = np.s_[f0:f0 + wf_len, y0:y0 + th, x0:x0 + tw]
        direct = alpha[0][:, None, None] * alpha[1][None, :, None] * alpha[2][None, None, :] / raw[sel]
        prod = pl.wf[kf].astype(np.float64)[:, None, None] * pl.wy[ky].astype(np.float64)[None, :, None] * pl.wx[kx].astype(np.float64)[None, None, :]
        assert np.abs(prod / direct - 1.0).max() <= 4 * 2.0 ** -24
    assert np.array_equal(count, pl.coverage()) and count.min() >= 1
    assert pl.y.coverage().max() <= -(-th // sy) and pl.x.coverage().max() <= -(-tw // sx)
    assert count.max() <= tm.max_coverage(shape)


ILLEGAL = [((7, 12), (4, 8), (2, 4), "y (total=7, tile=4, stride=2)", "6 and 8"),
           ((6, 13), (4, 8), (2, 4), "x (total=13, tile=8, stride=4)", "12 and 16"),
           ((6, 12), (4, 8), (5, 4), "y (total=6, tile=4, stride=5)", "stride must be from 1 to tile"),
           ((6, 12), (4, 8), (2, 0), "x (total=12, tile=8, stride=0)", "stride must be from 1 to tile"),
           ((3, 12), (4, 8), (2, 4), "y (total=3, tile=4, stride=2)", "at least tile"),
           ((6, 12), (4, 0), (2, 4), "x (total=12, tile=0, stride=4)", "at least 1")]


@pytest.mark.parametrize("case", ILLEGAL, ids=[c[3] for c in ILLEGAL])
def test_illegal_triples_raise_naming_axis_and_numbers(case):
    from vdpp_amd.models import tile_plan
    (h, w), tile, stride, names, says = case
    with pytest.raises(ValueError) as err:
        tile_plan.plan(h, w, tile, stride)
    assert names in str(err.value) and says in str(err.value), str(err.value)


def test_other_plan_errors_and_noise_shape():
    from vdpp_amd.models import tile_plan, window_plan
    assert tile_plan.legal_totals is window_plan.legal_totals and tile_plan.legal_totals(13, 8, 4) == (12, 16)
    assert tile_plan.legal_totals(12, 8, 4) == (12, 12) and tile_plan.legal_totals(5, 8, 4) == (8, 8)
    with pytest.raises(ValueError, match="tile_weights"):
        tile_plan.plan(6, 12, (4, 8), (2, 4), "gauss")
    with pytest.raises(ValueError, match="tile_size must be a pair"):
        tile_plan.plan(6, 12, 4, (2, 4))
    with pytest.raises(ValueError, match="tile_stride must be a pair"):
        tile_plan.plan(6, 12, (4, 8), (2, 4, 1))
    with pytest.raises(ValueError, match=r"frames_total=7, window=4, stride=2.*6 and 8"):
        tile_plan.plan(6, 12, (4, 8), (2, 4), frames_total=7, window=4, window_stride=2)
    assert tile_plan.noise_shape(2, 5, 64, 192, 64, 128, 64, 64) == (2, 4, 5, 8, 24)
    with pytest.raises(ValueError, match=r"x \(total=25, tile=16, stride=8\).*24 and 32"):
        tile_plan.noise_shape(1, 5, 64, 200, 64, 128, 64, 64)
    with pytest.raises(ValueError, match="multiple of 8"):
        tile_plan.noise_shape(1, 5, 64, 196, 64, 128, 64, 64)


@pytest.mark.parametrize("weights", ["triangle", "uniform"])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("shape", tm.SHAPES, ids=tm.SHAPE_IDS)
def test_patches_that_agree_give_the_plain_step(shape, guided, weights):
    """Every patch reports the same eps for an element (guidance 1.0 when guided): the tiled step is the plain step on the
    large latent, to 1e-12."""
    from tests import solver_model as sm
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    rng = np.random.default_rng(ft + 31 * sy + w)
    pl = _plan(h, w, (th, tw), (sy, sx), weights, frames_total=ft, window=wf, window_stride=sf)
    plain_c = rng.standard_normal((nb, ft, h, w, 4)).astype(np.float16)
    plain_u = rng.standard_normal((nb, ft, h, w, 4)).astype(np.float16) if guided else None

    def tiled(rows):
        return None if rows is None else np.concatenate(
            [rows[:, f0:f0 + wf, y0:y0 + th, x0:x0 + tw].reshape(-1, 4) for *_, f0, y0, x0 in pl.patches()])

    g_w, g_f = (np.ones(wf, np.float32), np.ones(ft, np.float32)) if guided else (None, None)
    state = (rng.standard_normal((nb, 8, ft, h, w)) * 3).astype(np.float16)
    kw = dict(sigma=1.7, a=0.6, b=0.4, c1=1.3, c2=0.3)
    x_new, d, _, _ = tm.dpmpp2m_step_tiles(state, tiled(plain_c), tiled(plain_u), g_w, shape=shape, weights=weights, **kw)
    want_x, want_d, _ = sm.dpmpp2m_step(state, plain_c.reshape(-1, 4), None if plain_u is None else plain_u.reshape(-1, 4), g_f, **kw)
    assert np.abs(x_new - want_x).max() <= 1e-12 and np.abs(d - want_d).max() <= 1e-12


def test_one_tile_is_the_window_model():
    """One tile that is the whole frame: the statement is ``window_model``'s, value for value, with and without frame windows;
    the bound is never below the window bound."""
    for frames in ((6, 4, 2), (3, 3, 3)):
        shape = (2,) + frames + (3, 5, 3, 5, 2, 4)
        state, ec, eu, g, _ = tm.case_inputs(shape, 8, "per-video", channels=8, sigma=2.0)
        kw = dict(sigma=2.0, a=0.5, b=0.5, c1=1.25, c2=0.25)
        x_new, d, terms, d_terms = tm.dpmpp2m_step_tiles(state, ec, eu, g, shape=shape, **kw)
        want = wm.dpmpp2m_step_windows(state, ec, eu, g, window=frames[1], stride=frames[2], **kw)
        for a, b in zip((x_new, d, terms, d_terms), want):
            assert np.array_equal(a, b)
        assert (tm.bound(x_new, terms, shape) >= wm.bound(x_new, terms, frames[1], frames[2])).all()


# the mistakes that are no mistake on some inputs: disjoint tiles all carry weight 1 and no element has a second patch
def _applies(bug, shape):
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    disjoint = sy == th and sx == tw and sf == wf
    return not (disjoint and bug in ("no_weights", "last_overwrites", "swap_wy_wx"))


@pytest.mark.parametrize("bug", tm.BUGS)
def test_planted_bugs_leave_the_kernel_bound(bug):
    """On the inputs of ``test_tile_gpu.py::test_kernels_against_the_fp64_model`` -- both ``ld_eps``, the three guidance modes,
    both sampler steps -- every planted mistake moves x' (and D) past TWICE the bound the kernels are held to, at every shape
    where it is a mistake at all."""
    checked = 0
    for shape in tm.SHAPES:
        if not _applies(bug, shape):
            continue
        for ld_eps in (4, 8):
            for guidance in ("none", "shared", "per-video"):
                for name, step in wm.kernel_steps().items():
                    euler, coef = wm.split_step(step)
                    what = (bug, shape, ld_eps, guidance, name)
                    state, ec, eu, g, _ = tm.case_inputs(shape, ld_eps, guidance, channels=8, sigma=step["sigma"],
                                                         nan_history=name == "first-order")
                    good_x, good_d, terms, d_terms = tm.dpmpp2m_step_tiles(state, ec, eu, g, shape=shape, **coef)
                    bad_x, bad_d, _, _ = tm.dpmpp2m_step_tiles(state, ec, eu, g, shape=shape, bug=bug, **coef)
                    assert (np.abs(bad_x - good_x) / tm.bound(good_x, terms, shape)).max() > 2.0, what + ("2M x'",)
                    assert (np.abs(bad_d - good_d) / tm.bound(good_d, d_terms, shape)).max() > 2.0, what + ("2M D",)
                    lat, ec, eu, g, _ = tm.case_inputs(shape, ld_eps, guidance, channels=4, sigma=step["sigma"])
                    good, terms = tm.euler_step_tiles(lat, ec, eu, g, shape=shape, **euler)
                    bad, _ = tm.euler_step_tiles(lat, ec, eu, g, shape=shape, bug=bug, **euler)
                    assert (np.abs(bad - good) / tm.bound(good, terms, shape)).max() > 2.0, what + ("Euler",)
                    checked += 1
    assert checked >= 36


def test_generate_takes_the_tile_options_and_names_what_is_wrong(capsys):
    from vdpp_amd.modes import generate
    base = ["--random-init", "--input-image", "in.png", "--output", "out.gif"]
    tiles = ["--tile-height", "64", "--tile-width", "128", "--tile-stride-y", "64", "--tile-stride-x", "64"]
    a = generate.parse_args(base)
    assert a.tile_height is None and a.tile_weights == "triangle" and generate.tile_arguments(a) == {}
    a = generate.parse_args(base + ["--height", "64", "--width", "192", "--tile-weights", "uniform"] + tiles)
    assert generate.tile_arguments(a) == dict(tile_size=(8, 16), tile_stride=(8, 8), tile_weights="uniform")

    def refused(argv, *texts):
        with pytest.raises(SystemExit) as err:
            generate.parse_args(base + argv)
        assert err.value.code == 2
        said = capsys.readouterr().err
        for t in texts:
            assert t in said, said

    refused(["--tile-height", "64"], "go together")
    refused(["--height", "64", "--width", "200"] + tiles, "--width 200", "--tile-width 128", "192 and 256")
    refused(["--height", "96", "--width", "192"] + tiles, "--height 96", "64 and 128")
    refused(["--height", "64", "--width", "64"] + tiles, "--width 64 is less than --tile-width 128", "128 and 192")
    refused(["--height", "64", "--width", "192"] + tiles[:-1] + ["136"], "--tile-stride-x 136 must be from 8 to --tile-width 128")
    refused(["--height", "64", "--width", "192"] + tiles[:-1] + ["0"], "--tile-stride-x 0 must be from 8")
    refused(["--height", "64", "--width", "192"] + tiles[:-1] + ["60"], "multiples of 8")
    refused(["--height", "64", "--width", "192", "--tile-weights", "gauss"] + tiles, "--tile-weights")
