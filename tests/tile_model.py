"""Large frames as overlapping spatial tiles in fp64 numpy: what ``sp_euler_step_tiles_f16`` and ``sp_dpmpp2m_step_tiles_f16``
(csrc/sampler_tail.hip) and ``models/tile_plan.py`` are held to.

Plan: per axis the rule of ``window_model.plan`` -- total ``T``, tile ``t``, stride ``s``, ``n = (T - t)/s + 1`` tiles, tile ``k``
covering cells ``k*s .. k*s + t - 1``, normalised fp64 table ``[n][t]``.  A patch is (frame window ``kf``, tile ``ky``, tile
``kx``), patch ``k = (kf*n_ty + ky)*n_tx + kx``, its weight at global (f, y, x) the product of the three tables' values.  The
product profile's normaliser is the product of the per-axis normalisers, so the product of the normalised tables IS the
normalised product profile (``test_tile_cpu.py`` checks it).

Layouts as the kernels': latent ``(B, 4, F_total, H, W)`` / state ``(B, 8, F_total, H, W)``; eps rows
``[n_patch][B][Wf][th*tw][ld_eps]``; guidance ``None``, ``[Wf]`` or ``[B][>= Wf]``, indexed by the position in the frame window.
Per patch the guidance mix is evaluated in fp16 (``solver_model.guidance_mix_f16``); the fusion and the update in fp64.

Bound, every output of the kernels: ``1 fp16 ulp of the model value + (8 + 6*C) * 2^-24 * terms`` with
``C = ceil(Wf/Sf) * ceil(th/sy) * ceil(tw/sx)``, the most patches that can cover an element, and ``terms`` the sum of
magnitudes of ``window_model`` with each patch's weighted eps counted as one.  It is the single-window bound
(``solver_model.bound``) with six more roundings per covering patch: the three tables' roundings to fp32, the two products
``(wf*wy)*wx`` and the ``fmaf`` into the sum; each is relative to a value that the partial sum of magnitudes bounds.

``bug=`` plants one mistake (``BUGS``); ``test_tile_cpu.py`` shows that each leaves twice the bound on the kernel-test inputs.
"""

from __future__ import annotations

import math

import numpy as np

from tests import solver_model as sm
from tests import window_model as wm

BUGS = ("unnormalised", "swap_wy_wx", "x_start_off_by_one", "drop_last_y", "no_weights", "tile0_rows", "row_large_w",
        "last_overwrites")

# (B, F_total, Wf, Sf, H, W, th, tw, sy, sx) of the kernel tests: even coverage in the four-pixel form; coverage 3 x 2, uneven,
# one pixel per thread; disjoint tiles; the product plan with two frame windows
SHAPES = [(2, 3, 3, 3, 6, 12, 4, 8, 2, 4), (2, 2, 2, 2, 5, 7, 3, 3, 1, 2), (2, 2, 2, 2, 4, 8, 2, 4, 2, 4),
          (1, 6, 4, 2, 6, 12, 4, 8, 2, 4)]
SHAPE_IDS = ["even-coverage-four-pixels", "uneven-coverage-one-pixel", "disjoint-tiles", "product-plan-two-windows"]


def plans(shape, weights="triangle"):
    """``((f starts, wf), (y starts, wy), (x starts, wx))``, fp64 tables."""
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    return wm.plan(ft, wf, sf, weights), wm.plan(h, th, sy, weights), wm.plan(w, tw, sx, weights)


def n_patch(shape):
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    return ((ft - wf) // sf + 1) * ((h - th) // sy + 1) * ((w - tw) // sx + 1)


def max_coverage(shape):
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    return math.ceil(wf / sf) * math.ceil(th / sy) * math.ceil(tw / sx)


def patch_eps(eps_cond, eps_uncond, guidance, shape):
    """Every patch's eps after the fp16 guidance mix: fp64 ``[n_patch][B][4][Wf][th][tw]``."""
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    return wm.window_eps(eps_cond, eps_uncond, guidance, nb=nb, n_win=n_patch(shape), window=wf, h=th, w=tw)


def _covers(starts, tile, total, *, shift=0, drop_last=False):
    """Per tile of one axis ``(global cells it contributes to, their index inside the tile)``."""
    out = []
    for s in starts:
        cells = np.array([c for c in range(total) if s + shift <= c < s + shift + tile], dtype=np.int64)
        if drop_last:   # a cell loses the last tile that covers it
            last = {c: max(s2 for s2 in starts if s2 <= c < s2 + tile) for c in range(total)}
            cells = np.array([c for c in cells if last[c] != s], dtype=np.int64)
        out.append((cells, cells - s - shift))
    return out


def fuse(e_k, shape, *, weights="triangle", bug=None):
    """``(e, abs_e)``: the fused prediction ``(B, 4, F_total, H, W)`` and the sum of its terms' magnitudes, patches added with
    ``kf`` ascending outermost, then ``ky``, then ``kx``."""
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    (fs, tf), (ys, ty), (xs, tx) = plans(shape, weights)
    if bug == "unnormalised":
        ty, tx = np.broadcast_to(wm.profile(th, weights), ty.shape), np.broadcast_to(wm.profile(tw, weights), tx.shape)
    if bug == "no_weights":
        tf, ty, tx = np.ones_like(tf), np.ones_like(ty), np.ones_like(tx)
    if bug == "tile0_rows":       # every tile of a frame window reads the rows of that window's tile (0, 0)
        per_win = len(ys) * len(xs)
        e_k = np.stack([e_k[k // per_win * per_win] for k in range(e_k.shape[0])])
    if bug == "row_large_w":      # the row inside a tile from the LATENT's row length: ly*W + lx, not ly*tw + lx
        rows = e_k.transpose(0, 1, 3, 4, 5, 2).reshape(-1, 4)                       # [n_patch][B][Wf][th*tw] rows
        base = np.arange(e_k.shape[0] * nb * wf).reshape(e_k.shape[0], nb, wf, 1, 1) * (th * tw)
        idx = (base + np.arange(th).reshape(1, 1, 1, th, 1) * w + np.arange(tw).reshape(1, 1, 1, 1, tw)) % rows.shape[0]
        e_k = rows[idx].transpose(0, 1, 5, 2, 3, 4)
    cf = _covers(fs, wf, ft)
    cy = _covers(ys, th, h, drop_last=bug == "drop_last_y")
    cx = _covers(xs, tw, w, shift=1 if bug == "x_start_off_by_one" else 0)
    e = np.zeros((nb, 4, ft, h, w))
    abs_e = np.zeros_like(e)
    for kf, (gf, lf) in enumerate(cf):
        for ky, (gy, ly) in enumerate(cy):
            for kx, (gx, lx) in enumerate(cx):
                if not (len(gf) and len(gy) and len(gx)):
                    continue
                k = (kf * len(ys) + ky) * len(xs) + kx
                if bug == "swap_wy_wx":      # the y table read along x and the x table along y (indices wrapped into the tables)
                    wgt = tf[kf][lf][:, None, None] * tx[ky % len(xs)][ly % tw][None, :, None] * ty[kx % len(ys)][lx % th][None, None, :]
                else:
                    wgt = tf[kf][lf][:, None, None] * ty[ky][ly][None, :, None] * tx[kx][lx][None, None, :]
                sel = np.ix_(range(nb), range(4), gf, gy, gx)
                src = e_k[k][np.ix_(range(nb), range(4), lf, ly, lx)]
                if bug == "last_overwrites":
                    e[sel] = src
                    continue
                e[sel] += wgt * src
                abs_e[sel] += np.abs(wgt * src)
    return e, abs_e


def _fused(eps_cond, eps_uncond, guidance, shape, weights, bug):
    return fuse(patch_eps(eps_cond, eps_uncond, guidance, shape), shape, weights=weights, bug=bug)


def euler_step_tiles(latent, eps_cond, eps_uncond, guidance, *, shape, sigma, sigma_next, weights="triangle", bug=None):
    """``(x', terms)`` as ``window_model.euler_step_windows``, each patch's weighted eps counted as a term."""
    x = np.asarray(latent).astype(np.float64)
    e, abs_e = _fused(eps_cond, eps_uncond, guidance, shape, weights, bug)
    s = float(sigma)
    c_skip, c_out = 1.0 / (s * s + 1.0), -s / math.sqrt(s * s + 1.0)
    r = (float(sigma_next) - s) / s
    terms = np.abs(x) + abs(r) * (np.abs(x) + np.abs(c_skip * x) + abs(c_out) * abs_e)
    return sm.euler_step(x, e, s, sigma_next), terms


def dpmpp2m_step_tiles(state, eps_cond, eps_uncond, guidance, *, shape, sigma, a, b, c1, c2, weights="triangle", bug=None):
    """``(x', D, terms, d_terms)`` as ``window_model.dpmpp2m_step_windows``."""
    state = np.asarray(state)
    assert state.shape[1] == 8
    x = state[:, :4].astype(np.float64)
    e, abs_e = _fused(eps_cond, eps_uncond, guidance, shape, weights, bug)
    s = float(sigma)
    c_skip, c_out = 1.0 / (s * s + 1.0), -s / math.sqrt(s * s + 1.0)
    d = sm.denoised(x, e, s)
    d_terms = np.abs(c_skip * x) + abs(c_out) * abs_e
    hist = np.zeros_like(d) if c2 == 0.0 else c2 * state[:, 4:].astype(np.float64)
    x_new = a * x + b * (c1 * d - hist)
    terms = np.abs(a * x) + abs(b * c1) * d_terms + np.abs(b * hist)
    return x_new, d, terms, d_terms


def bound(model_value, terms, shape, nz=0.0):
    """``1 fp16 ulp + (8 + 6*C) * 2^-24 * terms`` (the module's docstring), plus ``2^-19 * |n*z|`` for a stochastic step
    (``noise_model.bound``; ``terms`` then includes ``|n*z|``)."""
    return sm.fp16_ulp(model_value) + (8.0 + 6.0 * max_coverage(shape)) * 2.0 ** -24 * terms + 2.0 ** -19 * nz


def window_shape(shape):
    """The ``(B, F_total, Wf, Sf, H, W)`` of ``window_model`` / ``noise_model`` for the large latent."""
    return tuple(shape[:6])


def case_inputs(shape, ld_eps, guidance, *, channels, sigma, nan_history=False, seed=0):
    """The inputs of one kernel case, the same in the CPU and the GPU test: ``(state fp16, eps_cond, eps_uncond, guidance,
    ld_guidance)``.  eps columns past the four real channels and the pad of per-video guidance rows hold NaN; the patches of
    one element get unrelated eps, so every mistake in which patch goes where shows."""
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    rng = np.random.default_rng(7919 * seed + 1000 * ld_eps + 10 * len(guidance) + 97 * ft + 13 * h + w + 3 * sx)
    x = rng.standard_normal((nb, 4, ft, h, w)) * (float(sigma) + 1.0)
    if channels == 8:
        old = np.full_like(x, np.nan) if nan_history else rng.standard_normal((nb, 4, ft, h, w))
        x = np.concatenate([x, old], axis=1)
    n = n_patch(shape) * nb * wf * th * tw

    def rows():
        v = np.full((n, ld_eps), np.nan)
        v[:, :4] = rng.standard_normal((n, 4))
        return v.astype(np.float16)

    g, ld_g = wm.guidance_rows(guidance, nb, wf)
    ec = rows()
    eu = rows() if g is not None else None
    return x.astype(np.float16), ec, eu, g, ld_g
