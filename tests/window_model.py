"""Long videos as overlapping frame windows in fp64 numpy: what ``sp_euler_step_windows_f16`` and
``sp_dpmpp2m_step_windows_f16`` (csrc/sampler_tail.hip) and ``models/window_plan.py`` are held to.

Plan: ``n_win = (F_total - W)/S + 1`` windows, window ``k`` covers global frames ``k*S .. k*S + W - 1``; profile
``alpha(p) = min(p + 1, W - p)`` ("triangle") or 1 ("uniform"); ``wn[k][p] = alpha(p) / sum over the windows k' covering
f = k*S + p of alpha(f - k'*S)`` in fp64.  The kernels are given the table rounded to fp32; that rounding is theirs (one of the
two roundings per window the bound allows), the statement keeps fp64.

Layouts as the kernels': latent ``(B, 4, F_total, H, W)`` / state ``(B, 8, F_total, H, W)``; eps rows
``[n_win][B][W][H*W][ld_eps]`` with the four real channels in front; guidance ``None``, ``[W]`` or ``[B][>= W]``, indexed by the
position in the window.  Per window the guidance mix is evaluated in fp16 (``solver_model.guidance_mix_f16``); the fusion
``e(f) = sum_k wn[k][f - k*S] * e_k[f - k*S]`` and the update behind it in fp64.  Nothing is rounded at the end.

``bug=`` plants one mistake a kernel or its caller could make (``BUGS``); ``test_window_cpu.py`` shows that each moves the
result past twice the kernel bound on the inputs of the GPU test.
"""

from __future__ import annotations

import math

import numpy as np

from tests import solver_model as sm

BUGS = ("unnormalised", "guidance_global", "start_off_by_one", "drop_last", "no_weights", "uncond_window0", "last_overwrites")

# (B, F_total, W, S, h, w) of the kernel tests: even coverage, uneven coverage, disjoint windows, the one-pixel path with
# coverage 4 (H*W = 15)
SHAPES = [(1, 8, 4, 2, 8, 8), (2, 10, 4, 3, 8, 8), (2, 8, 4, 4, 8, 8), (1, 7, 4, 1, 3, 5)]


def profile(window, weights="triangle"):
    p = np.arange(window, dtype=np.float64)
    if weights == "triangle":
        return np.minimum(p + 1.0, window - p)
    if weights == "uniform":
        return np.ones(window)
    raise ValueError(weights)


def plan(frames_total, window, stride, weights="triangle"):
    """``(starts, table)``: the first global frame of every window and the fp64 ``[n_win][W]`` weights."""
    if window < 1 or frames_total < window or not 1 <= stride <= window or (frames_total - window) % stride:
        raise ValueError(f"illegal window plan ({frames_total}, {window}, {stride})")
    starts = [k * stride for k in range((frames_total - window) // stride + 1)]
    alpha = profile(window, weights)
    table = np.zeros((len(starts), window))
    for k, s in enumerate(starts):
        for p in range(window):
            f = s + p
            table[k, p] = alpha[p] / sum(alpha[f - s2] for s2 in starts if s2 <= f < s2 + window)
    return starts, table


def max_coverage(window, stride):
    return math.ceil(window / stride)


def window_eps(eps_cond, eps_uncond, guidance, *, nb, n_win, window, h, w, frames_total=None, stride=None, bug=None):
    """Every window's eps after the fp16 guidance mix: fp64 ``[n_win][B][4][W][h][w]``."""
    ec = np.asarray(eps_cond)[:, :4].reshape(n_win, nb, window, h, w, 4).transpose(0, 1, 5, 2, 3, 4)
    if eps_uncond is None:
        return ec.astype(np.float64)
    eu = np.asarray(eps_uncond)[:, :4].reshape(n_win, nb, window, h, w, 4).transpose(0, 1, 5, 2, 3, 4)
    if bug == "uncond_window0":
        eu = np.broadcast_to(eu[:1], eu.shape)
    g = np.asarray(guidance, np.float32)
    g = np.broadcast_to(g.reshape(1, -1) if g.ndim == 1 else g, (nb, g.shape[-1]))[:, :window]
    out = np.empty(ec.shape, dtype=np.float64)
    for k in range(n_win):
        gk = g
        if bug == "guidance_global":
            # the scale ramp of a window stretched over the whole video and read at the global frame: what a caller makes who
            # prepares guidance for F_total frames.  This is NOT the literal index mistake (row[k*S + p] on a [W] row): that
            # one reads past the row, has no model value, and is caught in the GPU test by the NaN pad of the per-video
            # rows alone (the result must be finite); a shared [W] row has no pad to catch it.
            pos = (k * stride + np.arange(window)) * (window - 1.0) / (frames_total - 1.0)
            gk = np.stack([np.interp(pos, np.arange(window), row) for row in g]).astype(np.float32)
        out[k] = sm.guidance_mix_f16(ec[k], eu[k], gk.reshape(nb, 1, window, 1, 1)).astype(np.float64)
    return out


def fuse(e_k, starts, table, frames_total, *, window, weights="triangle", bug=None):
    """``(e, abs_e)``: the fused prediction ``(B, 4, F_total, h, w)`` and the sum of its terms' magnitudes."""
    n_win, nb, _, _, h, w = e_k.shape
    wn = np.asarray(table, np.float64)
    if bug == "unnormalised":
        wn = np.broadcast_to(profile(window, weights), wn.shape)
    if bug == "no_weights":
        wn = np.ones_like(wn)
    shift = 1 if bug == "start_off_by_one" else 0
    e = np.zeros((nb, 4, frames_total, h, w))
    abs_e = np.zeros_like(e)
    for f in range(frames_total):
        cover = [k for k, s in enumerate(starts) if s + shift <= f < s + shift + window]
        if bug == "drop_last":
            cover = cover[:-1]
        if bug == "last_overwrites":
            if cover:
                e[:, :, f] = e_k[cover[-1], :, :, f - starts[cover[-1]]]
            continue
        for k in cover:
            term = wn[k, f - starts[k] - shift] * e_k[k, :, :, f - starts[k] - shift]
            e[:, :, f] += term
            abs_e[:, :, f] += np.abs(term)
    return e, abs_e


def _fused(x_shape, eps_cond, eps_uncond, guidance, *, window, stride, weights, bug):
    nb, _, ft, h, w = x_shape
    starts, table = plan(ft, window, stride, weights)
    e_k = window_eps(eps_cond, eps_uncond, guidance, nb=nb, n_win=len(starts), window=window, h=h, w=w, frames_total=ft,
                     stride=stride, bug=bug)
    return fuse(e_k, starts, table, ft, window=window, weights=weights, bug=bug)


def euler_step_windows(latent, eps_cond, eps_uncond, guidance, *, sigma, sigma_next, window, stride, weights="triangle",
                       bug=None):
    """``(x', terms)``: ``x + (x - (c_skip*x + c_out*e))/sigma * (sigma_next - sigma)`` and the magnitudes its fp32 evaluation
    scales with, each window's weighted eps counted as a term."""
    x = np.asarray(latent).astype(np.float64)
    e, abs_e = _fused(x.shape, eps_cond, eps_uncond, guidance, window=window, stride=stride, weights=weights, bug=bug)
    s = float(sigma)
    c_skip, c_out = 1.0 / (s * s + 1.0), -s / math.sqrt(s * s + 1.0)
    r = (float(sigma_next) - s) / s
    x_new = sm.euler_step(x, e, s, sigma_next)
    terms = np.abs(x) + abs(r) * (np.abs(x) + np.abs(c_skip * x) + abs(c_out) * abs_e)
    return x_new, terms


def dpmpp2m_step_windows(state, eps_cond, eps_uncond, guidance, *, sigma, a, b, c1, c2, window, stride, weights="triangle",
                         bug=None):
    """``(x', D, terms, d_terms)``: ``D = c_skip*x + c_out*e``, ``x' = a*x + b*(c1*D - c2*D_prev)``; ``d_terms`` the
    magnitudes of D's terms, ``terms`` those of x' (D's inside ``b*c1``)."""
    state = np.asarray(state)
    assert state.shape[1] == 8
    x = state[:, :4].astype(np.float64)
    e, abs_e = _fused(x.shape, eps_cond, eps_uncond, guidance, window=window, stride=stride, weights=weights, bug=bug)
    s = float(sigma)
    c_skip, c_out = 1.0 / (s * s + 1.0), -s / math.sqrt(s * s + 1.0)
    d = sm.denoised(x, e, s)
    d_terms = np.abs(c_skip * x) + abs(c_out) * abs_e
    hist = np.zeros_like(d) if c2 == 0.0 else c2 * state[:, 4:].astype(np.float64)
    x_new = a * x + b * (c1 * d - hist)
    terms = np.abs(a * x) + abs(b * c1) * d_terms + np.abs(b * hist)
    return x_new, d, terms, d_terms


def bound(model_value, terms, window, stride):
    """``1 fp16 ulp of the model value + (8 + 2*ceil(W/S)) * 2^-24 * terms``: ``solver_model.bound`` with two more roundings
    per window that can cover a frame -- its weight's rounding to fp32 and its fmaf."""
    return sm.fp16_ulp(model_value) + (8.0 + 2.0 * max_coverage(window, stride)) * 2.0 ** -24 * terms


# ------------------------------------------------------------------------------------------------ shared inputs
def kernel_steps(n_steps=25):
    """The sampler steps of the kernel tests, ``name -> dict(sigma, sigma_next, a, b, c1, c2)``: step 12 of the 25-step Karras
    table with its own second-order coefficients ("history") and step 0 (sigma = 700, ``c2 == 0``: "first-order").  The sigmas
    are the fp32 table's values, so the kernels' float arguments hold them exactly."""
    from vdpp_amd.models.euler_schedule import karras_sigma_table
    from vdpp_amd.models.solver_schedule import dpmpp_2m_coefficients
    sig32 = karras_sigma_table(n_steps)
    coef, sig = dpmpp_2m_coefficients(sig32), sig32.double().tolist()
    out = {}
    for name, step in (("history", 12), ("first-order", 0)):
        a, b, c1, c2 = coef[step]
        assert (c2 > 0) == (name == "history")
        out[name] = dict(sigma=sig[step], sigma_next=sig[step + 1], a=a, b=b, c1=c1, c2=c2)
    return out


def split_step(step):
    """``(euler kwargs, 2M kwargs)`` of one ``kernel_steps`` entry."""
    return ({k: step[k] for k in ("sigma", "sigma_next")}, {k: step[k] for k in ("sigma", "a", "b", "c1", "c2")})


def guidance_rows(mode, nb, window, ld=None):
    """``(guidance, ld_guidance)`` for ``mode`` in "none", "shared" (one ``[W]`` row), "per-video" (``[B][ld]`` with
    ``ld = W + 3 > W``: the pad holds NaN, a kernel that indexes past the window reads it)."""
    if mode == "none":
        return None, 0
    if mode == "shared":
        return np.linspace(1.0, 3.0, window).astype(np.float32), 0
    ld = window + 3 if ld is None else ld
    rows = np.full((nb, ld), np.nan, dtype=np.float32)
    for i, g in enumerate([3.0, 2.0][:nb]):
        rows[i, :window] = np.linspace(1.0, g, window)
    return rows, ld


def case_inputs(shape, ld_eps, guidance, *, channels, sigma, nan_history=False, seed=0):
    """The inputs of one kernel case, the same in the CPU and the GPU test: ``(state fp16, eps_cond, eps_uncond, guidance,
    ld_guidance)``.  eps columns past the four real channels hold NaN (never read); windows of one global frame get unrelated
    eps, so every mistake in which window goes where shows."""
    nb, ft, window, stride, h, w = shape
    n_win = (ft - window) // stride + 1
    rng = np.random.default_rng(7919 * seed + 1000 * ld_eps + 10 * len(guidance) + 97 * ft + h)
    x = rng.standard_normal((nb, 4, ft, h, w)) * (float(sigma) + 1.0)
    if channels == 8:
        old = np.full_like(x, np.nan) if nan_history else rng.standard_normal((nb, 4, ft, h, w))
        x = np.concatenate([x, old], axis=1)
    n = n_win * nb * window * h * w

    def rows():
        v = np.full((n, ld_eps), np.nan)
        v[:, :4] = rng.standard_normal((n, 4))
        return v.astype(np.float16)

    g, ld_g = guidance_rows(guidance, nb, window)
    ec = rows()
    eu = rows() if g is not None else None
    return x.astype(np.float16), ec, eu, g, ld_g
