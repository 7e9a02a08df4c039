"""The DPM-Solver++(2M) update in fp64 numpy: what ``sp_dpmpp2m_step_rows_f16`` (csrc/sampler_tail.hip) is held to.

State layout as the kernel's: ``(B, 8, F, H, W)``, channels 0-3 the sample ``x``, channels 4-7 the previous step's denoised
estimate ``D_prev``; eps rows ``[B*F*H*W][ld_eps]`` with the four real channels in front; guidance ``None``, ``[F]`` (one row for
every video) or ``[B][F]``.  The guidance mix is evaluated in fp16, rounding for rounding as the reference's Euler step does
(``svd_unet.py:410-411``: fp16 tensors), everything behind it in fp64 on the fp16-stored inputs:

    e  = eps_u + g*(eps_c - eps_u)                  (fp16)
    D  = x/(sigma^2+1) - e*sigma/sqrt(sigma^2+1)
    x' = a*x + b*(c1*D - c2*D_prev)

With ``c2 == 0`` the history channels are not read (they may hold NaN).  Nothing is rounded at the end: the caller compares
against ``fp16_ulp`` of these values.
"""

from __future__ import annotations

import numpy as np


def guidance_mix_f16(eps_c, eps_u, g):
    """``eps_u + g*(eps_c - eps_u)`` with every operation rounded to fp16 (``g`` broadcasts against the rows)."""
    c, u = np.asarray(eps_c, np.float16), np.asarray(eps_u, np.float16)
    gh = np.asarray(g, np.float32).astype(np.float16)
    diff = (c.astype(np.float32) - u.astype(np.float32)).astype(np.float16)
    prod = (gh.astype(np.float32) * diff.astype(np.float32)).astype(np.float16)
    return (u.astype(np.float32) + prod.astype(np.float32)).astype(np.float16)


def rows_to_planes(rows, b, f, h, w):
    """eps rows ``[B*F*H*W][>= 4]`` -> ``(B, 4, F, H, W)``."""
    return np.asarray(rows)[:, :4].reshape(b, f, h, w, 4).transpose(0, 4, 1, 2, 3)


def denoised(x, e, sigma):
    """v-prediction: ``c_skip*x + c_out*e`` (fp64)."""
    s = float(sigma)
    return np.asarray(x, np.float64) / (s * s + 1.0) - np.asarray(e, np.float64) * (s / np.sqrt(s * s + 1.0))


def dpmpp2m_step(state, eps_cond, eps_uncond, guidance, *, sigma, a, b, c1, c2):
    """``(x', D, terms)``: the new sample and the denoised estimate, fp64 ``(B, 4, F, H, W)`` each, and
    ``|a*x| + |b*c1*D| + |b*c2*D_prev|``, the magnitude the kernel's fp32 roundings scale with."""
    state = np.asarray(state)
    nb, ch, f, h, w = state.shape
    assert ch == 8
    e = rows_to_planes(eps_cond, nb, f, h, w)
    if eps_uncond is not None:
        g = np.asarray(guidance, np.float32)
        g = np.broadcast_to(g.reshape(1, f) if g.ndim == 1 else g, (nb, f)).reshape(nb, 1, f, 1, 1)
        e = guidance_mix_f16(e, rows_to_planes(eps_uncond, nb, f, h, w), g)
    x = state[:, :4].astype(np.float64)
    d = denoised(x, e.astype(np.float64), sigma)
    if c2 == 0.0:
        hist = np.zeros_like(d)
    else:
        hist = c2 * state[:, 4:].astype(np.float64)
    x_new = a * x + b * (c1 * d - hist)
    terms = np.abs(a * x) + np.abs(b * c1 * d) + np.abs(b * hist)
    return x_new, d, terms


def fp16_ulp(v):
    """Spacing of fp16 at ``|v|`` (the subnormal spacing 2^-24 below 2^-14)."""
    v = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def bound(model_value, terms):
    """``1 fp16 ulp of the model value + 8 * 2^-24 * terms``: half an ulp for the final rounding of an exact result, the
    other half and the second term for the kernel's fp32 evaluation (a handful of roundings, each relative to one of the
    three products)."""
    return fp16_ulp(model_value) + 8.0 * 2.0 ** -24 * terms


def euler_step(x, e, sigma, sigma_next):
    """The reference's Euler update (``svd_unet.py:428-437``) in fp64, for the identity with ``c2 == 0``."""
    x = np.asarray(x, np.float64)
    s = float(sigma)
    x0 = denoised(x, e, s)
    return x + (x - x0) / s * (float(sigma_next) - s)
