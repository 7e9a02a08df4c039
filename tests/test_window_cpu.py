"""Long videos as overlapping frame windows, without a GPU: the host plan (``models/window_plan.py``) against the fp64 statement
(``tests/window_model.py``), the statement against itself, and the planted mistakes against the kernel bound of
``tests/test_window_gpu.py`` on that test's own inputs.

The consistency, one-window and planted-mistake tests hold ``tests/window_model.py`` against ``tests/solver_model.py`` and against
itself: what they prove is about the statement, not about product code.  They take the windows from ``models/window_plan.plan``
all the same, so that the statement they prove things about is the one the product plans by."""

import numpy as np
import pytest

from tests import solver_model as sm
from tests import window_model as wm

TRIPLES = [(8, 4, 2), (10, 4, 3), (8, 4, 4), (4, 4, 1), (7, 4, 1)]
ILLEGAL = [(9, 4, 2), (8, 4, 5), (8, 4, 0), (3, 4, 1), (10, 4, 4), (8, 0, 1)]


def _plan(*a, **kw):
    from vdpp_amd.models import window_plan
    return window_plan.plan(*a, **kw)


@pytest.mark.parametrize("weights", ["triangle", "uniform"])
@pytest.mark.parametrize("triple", TRIPLES)
def test_plan_properties(triple, weights):
    ft, w, s = triple
    pl = _plan(ft, w, s, weights)
    n_win = (ft - w) // s + 1
    assert pl.n_win == n_win and list(pl.starts) == [k * s for k in range(n_win)]
    assert pl.weights.dtype == np.float32 and pl.weights.shape == (n_win, w) and (pl.weights >= 0).all()
    total, count = np.zeros(ft), np.zeros(ft, dtype=int)
    for k, st in enumerate(pl.starts):
        total[st:st + w] += pl.weights[k].astype(np.float64)
        count[st:st + w] += 1
    assert np.abs(total - 1.0).max() <= 2.0 ** -22, total
    want = np.array([sum(1 for st in pl.starts if st <= f < st + w) for f in range(ft)])
    assert np.array_equal(count, want) and np.array_equal(pl.coverage(), want)
    assert 1 <= count.min() and count.max() <= wm.max_coverage(w, s)
    # the model's own plan, made another way, gives the same table
    starts, table = wm.plan(ft, w, s, weights)
    assert starts == list(pl.starts) and table.dtype == np.float64 and np.array_equal(table.astype(np.float32), pl.weights)
    if weights == "uniform":
        assert np.array_equal(pl.weights, np.stack([1.0 / want[st:st + w] for st in pl.starts]).astype(np.float32))
    if n_win == 1:
        assert np.array_equal(pl.weights, np.ones((1, w), dtype=np.float32))


@pytest.mark.parametrize("triple", ILLEGAL)
def test_illegal_triples_raise_naming_the_numbers(triple):
    from vdpp_amd.models import window_plan
    ft, w, s = triple
    with pytest.raises(ValueError) as err:
        window_plan.plan(ft, w, s)
    text = str(err.value)
    assert str(ft) in text and str(w) in text, text
    with pytest.raises(ValueError):
        wm.plan(ft, w, s)
    with pytest.raises(ValueError, match="window_weights"):
        window_plan.plan(8, 4, 2, "gauss")
    if w >= 1 and 1 <= s <= w and ft > w:
        lo, hi = window_plan.legal_totals(ft, w, s)
        assert lo < ft < hi and (lo - w) % s == 0 and hi - lo == s and f"{lo} and {hi}" in text
    assert window_plan.noise_shape(2, 8, 64, 128, 4, 2) == (2, 4, 8, 8, 16)
    with pytest.raises(ValueError):
        window_plan.noise_shape(1, 9, 64, 128, 4, 2)


@pytest.mark.parametrize("weights", ["triangle", "uniform"])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("shape", wm.SHAPES, ids=str)
def test_windows_that_agree_give_the_plain_step(shape, guided, weights):
    """Every window reports the same eps for a global frame (guidance 1.0 everywhere when guided, so that the position in the
    window does not matter): the windowed step is the plain step on F_total frames, to 1e-12."""
    nb, ft, w, s, h, ww = shape
    rng = np.random.default_rng(ft + 31 * s)
    starts = list(_plan(ft, w, s, weights).starts)
    plain_c = rng.standard_normal((nb, ft, h * ww, 4)).astype(np.float16)
    plain_u = rng.standard_normal((nb, ft, h * ww, 4)).astype(np.float16) if guided else None

    def windowed(rows):
        return None if rows is None else np.concatenate([rows[:, st:st + w] for st in starts]).reshape(-1, 4)

    g_w, g_f = (np.ones(w, np.float32), np.ones(ft, np.float32)) if guided else (None, None)
    state = (rng.standard_normal((nb, 8, ft, h, ww)) * 3).astype(np.float16)
    kw = dict(sigma=1.7, a=0.6, b=0.4, c1=1.3, c2=0.3)
    x_new, d, _, _ = wm.dpmpp2m_step_windows(state, windowed(plain_c), windowed(plain_u), g_w, window=w, stride=s,
                                             weights=weights, **kw)
    want_x, want_d, _ = sm.dpmpp2m_step(state, plain_c.reshape(-1, 4), None if plain_u is None else plain_u.reshape(-1, 4), g_f,
                                        **kw)
    assert np.abs(x_new - want_x).max() <= 1e-12 and np.abs(d - want_d).max() <= 1e-12
    e_new, _ = wm.euler_step_windows(state[:, :4], windowed(plain_c), windowed(plain_u), g_w, sigma=1.7, sigma_next=1.1,
                                     window=w, stride=s, weights=weights)
    e = sm.rows_to_planes(plain_c.reshape(-1, 4), nb, ft, h, ww)
    if guided:
        e = sm.guidance_mix_f16(e, sm.rows_to_planes(plain_u.reshape(-1, 4), nb, ft, h, ww), 1.0)
    assert np.abs(e_new - sm.euler_step(state[:, :4], e.astype(np.float64), 1.7, 1.1)).max() <= 1e-12


def test_one_window_is_the_single_window_model():
    nb, ft, h, w = 2, 4, 3, 5
    assert np.array_equal(_plan(ft, ft, 2).weights, np.ones((1, ft), dtype=np.float32))
    state, ec, eu, g, ld_g = wm.case_inputs((nb, ft, ft, 2, h, w), 8, "per-video", channels=8, sigma=2.0)
    kw = dict(sigma=2.0, a=0.5, b=0.5, c1=1.25, c2=0.25)
    x_new, d, terms, _ = wm.dpmpp2m_step_windows(state, ec, eu, g, window=ft, stride=2, **kw)
    want_x, want_d, want_t = sm.dpmpp2m_step(state, ec, eu, g[:, :ft], **kw)
    assert np.array_equal(x_new, want_x) and np.array_equal(d, want_d)
    assert (terms >= want_t * (1 - 1e-12)).all()          # (D's two terms counted apart: never less than |b*c1*D|)


# the mistakes that are no mistake on some inputs: without guidance nothing reads guidance or uncond rows; disjoint windows all
# carry weight 1
def _applies(bug, shape, guidance):
    nb, ft, w, s, h, ww = shape
    if bug in ("guidance_global", "uncond_window0") and guidance == "none":
        return False
    if bug == "no_weights" and s == w:
        return False
    return True


@pytest.mark.parametrize("bug", [b for b in wm.BUGS if b != "last_overwrites"])
def test_planted_bugs_leave_the_kernel_bound(bug):
    """On the inputs of ``test_window_gpu.py::test_kernels_against_the_fp64_model`` -- both ``ld_eps``, both sampler steps, the
    first-order one with NaN history -- every planted mistake moves x' (and D) past TWICE the bound the kernels are held to, at
    every shape and guidance mode where it is a mistake at all."""
    checked = 0
    for shape in wm.SHAPES:
        ft, w, s = shape[1], shape[2], shape[3]
        pl = _plan(ft, w, s)
        starts, table = wm.plan(ft, w, s)
        assert starts == list(pl.starts) and np.array_equal(table.astype(np.float32), pl.weights)
        for ld_eps in (4, 8):
            for guidance in ("none", "shared", "per-video"):
                if not _applies(bug, shape, guidance):
                    continue
                for name, step in wm.kernel_steps().items():
                    euler, coef = wm.split_step(step)
                    what = (bug, shape, ld_eps, guidance, name)
                    state, ec, eu, g, _ = wm.case_inputs(shape, ld_eps, guidance, channels=8, sigma=step["sigma"],
                                                         nan_history=name == "first-order")
                    good_x, good_d, terms, d_terms = wm.dpmpp2m_step_windows(state, ec, eu, g, window=w, stride=s, **coef)
                    bad_x, bad_d, _, _ = wm.dpmpp2m_step_windows(state, ec, eu, g, window=w, stride=s, bug=bug, **coef)
                    assert (np.abs(bad_x - good_x) / wm.bound(good_x, terms, w, s)).max() > 2.0, what + ("2M x'",)
                    assert (np.abs(bad_d - good_d) / wm.bound(good_d, d_terms, w, s)).max() > 2.0, what + ("2M D",)
                    lat, ec, eu, g, _ = wm.case_inputs(shape, ld_eps, guidance, channels=4, sigma=step["sigma"])
                    good, terms = wm.euler_step_windows(lat, ec, eu, g, window=w, stride=s, **euler)
                    bad, _ = wm.euler_step_windows(lat, ec, eu, g, window=w, stride=s, bug=bug, **euler)
                    assert (np.abs(bad - good) / wm.bound(good, terms, w, s)).max() > 2.0, what + ("Euler",)
                    checked += 1
    assert checked >= 24
