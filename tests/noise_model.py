"""The noise of the stochastic samplers in numpy: what ``csrc/noise.h``, ``sp_randn_f16``, ``sp_philox_blocks_u32`` and the
two stochastic tails (``sp_euler_ancestral_step_f16``, ``sp_dpmpp2m_sde_step_f16``) are held to.

Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", 2011; the Random123 / cuRAND
construction) on uint64 arrays that hold 32-bit words.  A round maps ``(c0, c1, c2, c3)`` to
``(hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0))`` and then bumps the key by ``(W0, W1)``; ten rounds.

Address: element ``(c, f, p)`` of a video's latent ``(4, F_total, H, W)`` has the flat index ``e = (c*F_total + f)*H*W + p``
(``f`` the GLOBAL frame); block ``j = e >> 2``, lane ``l = e & 3``; counter ``(j, step, purpose, 0)``, key
``(seed & 0xffffffff, seed >> 32)``; ``purpose`` 0 the initial noise (``step`` 0), 1 a sampler step's noise.

Normals: ``U(a) = ((a >> 9) + 0.5) * 2^-23``; ``z0 = r*cos(2*pi*U(u1))``, ``z1 = r*sin(2*pi*U(u1))`` with
``r = sqrt(-2 ln U(u0))``; ``z2``, ``z3`` the same from ``u2``, ``u3``.  Everything behind the integer words in fp64.

The two steps are ``window_model``'s with ``n*z`` added to the sample (``terms`` gains ``|n*z|``); unwindowed calls are one
window that is the whole latent.  ``bug=`` plants one mistake (``BUGS``); ``test_noise_cpu.py`` shows that each leaves at
least twice the step bound on the inputs of the GPU test.
"""

from __future__ import annotations

import numpy as np

from tests import solver_model as sm
from tests import window_model as wm

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
INITIAL, STEP = 0, 1          # purpose

BUGS = ("no_step", "seed_video0", "lane_window_local", "swap_words", "sigma_up_as_down", "noise_on_D", "purpose0")

# (B, F_total, W, S, h, w) of the step tests: four pixels per thread, one pixel per thread (H*W = 15), and the windows
# F_total = 5, W = 3, S = 2 in both forms
SHAPES = [(2, 3, 3, 3, 4, 4), (2, 3, 3, 3, 3, 5), (2, 5, 3, 2, 4, 4), (2, 5, 3, 2, 3, 5)]
SEEDS = (42, 2 ** 63 - 1)     # of the two videos of a step case


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays (or scalars) of 32-bit words; returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.asarray(k0, dtype=np.uint64) & MASK, np.asarray(k1, dtype=np.uint64) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def blocks(seed, j, step, purpose):
    """The words of blocks ``j`` (array) of one seed: uint32 ``[len(j)][4]``."""
    j = np.asarray(j, dtype=np.uint64)
    seed = int(seed)
    zero = np.zeros_like(j)
    out = philox4x32_10(j, zero + np.uint64(step), zero + np.uint64(purpose), zero, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(out, axis=-1).astype(np.uint32)


def uniform(a):
    """``((a >> 9) + 0.5) * 2^-23``: strictly inside (0, 1), exact in fp32 and here."""
    return ((np.asarray(a, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals_of_words(words, swap=False):
    """fp64 ``[...][4]`` normals of uint32 ``[...][4]`` words.  ``swap``: words 0/1 and 2/3 exchanged (a planted mistake)."""
    u = uniform(words)
    if swap:
        u = u[..., [1, 0, 3, 2]]
    z = np.empty(u.shape, dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., a]))
        z[..., a] = r * np.cos(2.0 * np.pi * u[..., a + 1])
        z[..., a + 1] = r * np.sin(2.0 * np.pi * u[..., a + 1])
    return z


def element_normals(seed, e, step, purpose, lane_e=None, swap=False):
    """The normals of the flat elements ``e`` (int array) of one video; ``lane_e``: take the lane from these indices."""
    e = np.asarray(e, dtype=np.int64)
    z4 = normals_of_words(blocks(seed, e.ravel() >> 2, step, purpose), swap=swap)
    lane = (e if lane_e is None else np.asarray(lane_e, dtype=np.int64)).ravel() & 3
    return z4[np.arange(e.size), lane].reshape(e.shape)


def video_normals(seed, frames, h, w, step, purpose):
    """``(4, F, h, w)``: every element of one video's latent."""
    return element_normals(seed, np.arange(4 * frames * h * w).reshape(4, frames, h, w), step, purpose)


def step_noise(seeds, shape, step, bug=None):
    """``z`` of a step for the latents ``(B, 4, F_total, h, w)`` of ``shape = (B, F_total, W, S, h, w)``."""
    nb, ft, window, stride, h, w = shape
    e = np.arange(4 * ft * h * w).reshape(4, ft, h, w)
    lane_e = None
    if bug == "lane_window_local":
        # the lane from the index inside the first window that covers the frame, a (4, W, h, w) latent
        c, f, p = np.meshgrid(np.arange(4), np.arange(ft), np.arange(h * w), indexing="ij")
        k_lo = np.where(f < window, 0, (f - window) // stride + 1)
        lane_e = ((c * window + (f - k_lo * stride)) * (h * w) + p).reshape(4, ft, h, w)
    out = np.empty((nb, 4, ft, h, w))
    for b in range(nb):
        seed = seeds[0] if bug == "seed_video0" else seeds[b]
        out[b] = element_normals(seed, e, 0 if bug == "no_step" else step, INITIAL if bug == "purpose0" else STEP,
                                 lane_e=lane_e, swap=bug == "swap_words")
    return out


def euler_ancestral_step(latent, eps_cond, eps_uncond, guidance, seeds, step, *, shape, sigma, sigma_down, n, bug=None):
    """``(x', terms, nz)``: the Euler step to ``sigma_down`` plus ``n*z``; ``terms`` the magnitudes its fp32 evaluation scales
    with, ``nz = |n*z|``.  ``bug="sigma_up_as_down"`` steps to ``n`` (= sigma_up for s_noise = 1) instead."""
    target = n if bug == "sigma_up_as_down" else sigma_down
    x, terms = wm.euler_step_windows(latent, eps_cond, eps_uncond, guidance, sigma=sigma, sigma_next=target, window=shape[2],
                                     stride=shape[3])
    nz = n * step_noise(seeds, shape, step, bug=bug)
    return x + nz, terms + np.abs(nz), np.abs(nz)


def dpmpp2m_sde_step(state, eps_cond, eps_uncond, guidance, seeds, step, *, shape, sigma, a, b, c1, c2, n, bug=None):
    """``(x', D, terms, d_terms, nz)``: ``x' = a*x + b*(c1*D - c2*D_prev) + n*z``; ``D`` carries no noise (with
    ``bug="noise_on_D"`` it does)."""
    x, d, terms, d_terms = wm.dpmpp2m_step_windows(state, eps_cond, eps_uncond, guidance, sigma=sigma, a=a, b=b, c1=c1, c2=c2,
                                                   window=shape[2], stride=shape[3])
    nz = n * step_noise(seeds, shape, step, bug=bug)
    if bug == "noise_on_D":
        d = d + nz
    return x + nz, d, terms + np.abs(nz), d_terms, np.abs(nz)


def bound(model_value, terms, nz, shape):
    """The deterministic step's bound -- ``solver_model.bound`` for one window that is the whole latent, else the window bound
    -- plus ``2^-19 * |n*z|``: sixteen fp32 ulps for the kernel's ``z`` (logf 3, sqrtf 3, sinpi / cospi 4, one product: 9 by the
    limits of the OpenCL profile the device library documents).  ``terms`` includes ``|n*z|``, so the rounding of ``n`` to
    fp32 and the fma are inside the first part."""
    nb, ft, window, stride, h, w = shape
    base = sm.bound(model_value, terms) if window == ft else wm.bound(model_value, terms, window, stride)
    return base + 2.0 ** -19 * nz


def z_interval_f16(z, scale=1.0):
    """``(lo, hi)`` fp16: where ``fp16(scale * z_kernel)`` may lie when ``|z_kernel - z| <= 2^-19 * |z|`` (rounding is monotone;
    the product's own rounding is one of the sixteen ulps)."""
    z = np.asarray(z, dtype=np.float64) * float(scale)
    a, b = z * (1.0 - 2.0 ** -19), z * (1.0 + 2.0 ** -19)
    return np.minimum(a, b).astype(np.float16), np.maximum(a, b).astype(np.float16)


def kernel_steps(n_steps=25, eta=1.0, s_noise=1.0):
    """The sampler steps of the kernel tests, ``name -> dict(step, sigma, euler=dict(sigma_down, n), sde=dict(a, b, c1, c2,
    n))``: step 12 of the 25-step Karras table ("history", ``c2 > 0``) and step 0 ("first-order", sigma = 700)."""
    from vdpp_amd.models.euler_schedule import karras_sigma_table
    from vdpp_amd.models.solver_schedule import dpmpp_2m_sde_coefficients, euler_ancestral_coefficients
    sig32 = karras_sigma_table(n_steps)
    sig = sig32.double().tolist()
    ea = euler_ancestral_coefficients(sig32, eta, s_noise)
    sde = dpmpp_2m_sde_coefficients(sig32, eta, s_noise)
    out = {}
    for name, step in (("history", 12), ("first-order", 0)):
        a, b, c1, c2, n = sde[step]
        assert (c2 > 0) == (name == "history")
        out[name] = dict(step=step, sigma=sig[step], euler=dict(sigma_down=ea[step][0], n=ea[step][1]),
                         sde=dict(a=a, b=b, c1=c1, c2=c2, n=n))
    return out
