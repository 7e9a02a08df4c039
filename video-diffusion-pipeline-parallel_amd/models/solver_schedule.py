"""Host-side coefficients of the DPM-Solver++(2M) sampler (``StableVideoUNet(sampler="dpmpp_2m")``).

k-diffusion's ``sample_dpmpp_2m`` (Lu et al., "DPM-Solver++", 2022; the multistep second-order variant) written in sigma:
with ``t = -ln(sigma)``, ``h = t' - t = ln(sigma / sigma')`` and ``exp(-h) = sigma' / sigma``, its update

    x' = (sigma'/sigma) * x - expm1(-h) * D_d,      D_d = (1 + 1/(2r)) * D - 1/(2r) * D_prev,   r = h_last / h

becomes ``x' = a*x + b*(c1*D - c2*D_prev)`` with the four per-step constants below.  The first step (no history) and the last
one (``sigma' = 0``, ``h`` infinite) are first order: ``c1 = 1, c2 = 0``, where ``x' = a*x + b*D`` is algebraically the Euler
step of the v-prediction schedule (``euler_schedule``) and, at ``sigma' = 0``, ``x' = D``.

``D_prev`` is the denoised estimate of step ``i - 1``: the sampler walks the sigma table in index order (0, 1, 2, ...).
The table is a few dozen numbers computed once on the host, in fp64.
"""

from __future__ import annotations

import math
from collections.abc import Sequence

SAMPLERS = ("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde")
STOCHASTIC = ("euler_a", "dpmpp_2m_sde")      # fresh noise at every step, from the videos' seeds (csrc/noise.h)


def _sigma_list(sigmas: Sequence[float]) -> list[float]:
    sig = [float(s) for s in (sigmas.tolist() if hasattr(sigmas, "tolist") else sigmas)]
    if len(sig) < 2:
        raise ValueError("a sigma table has at least two entries (one step)")
    for i in range(len(sig) - 1):
        if not (sig[i] > 0.0 and 0.0 <= sig[i + 1] < sig[i]):
            raise ValueError(f"sigmas must be positive and strictly decreasing (the last may be 0); got {sig[i]!r} -> "
                             f"{sig[i + 1]!r} at step {i}")
    return sig


def _noise_parameters(eta: float, s_noise: float) -> tuple[float, float]:
    eta, s_noise = float(eta), float(s_noise)
    if not (math.isfinite(eta) and eta >= 0.0 and math.isfinite(s_noise) and s_noise >= 0.0):
        raise ValueError(f"eta and s_noise must be finite and not negative; got eta={eta!r}, s_noise={s_noise!r}")
    return eta, s_noise


def dpmpp_2m_coefficients(sigmas: Sequence[float]) -> list[tuple[float, float, float, float]]:
    """One ``(a, b, c1, c2)`` per step for the sigma table ``sigmas`` (``N + 1`` entries, decreasing, the last may be 0).

    ``a = sigma'/sigma``, ``b = 1 - a``; ``c2 = h / (2*h_last)`` with ``h = ln(sigma/sigma')``, ``h_last =
    ln(sigma_prev/sigma)`` and ``c1 = 1 + c2``, except ``c1 = 1, c2 = 0`` at step 0 and where ``sigma' = 0``."""
    sig = _sigma_list(sigmas)
    out = []
    for i in range(len(sig) - 1):
        s, s_next = sig[i], sig[i + 1]
        a = s_next / s
        c2 = 0.0
        if i > 0 and s_next > 0.0:
            c2 = math.log(s / s_next) / (2.0 * math.log(sig[i - 1] / s))
        out.append((a, 1.0 - a, 1.0 + c2, c2))
    return out


def euler_ancestral_coefficients(sigmas: Sequence[float], eta: float = 1.0,
                                 s_noise: float = 1.0) -> list[tuple[float, float]]:
    """One ``(sigma_down, n)`` per step of the Euler ancestral sampler (k-diffusion's ``sample_euler_ancestral`` /
    ``get_ancestral_step``): the Euler step goes from ``sigma`` to ``sigma_down`` and ``n * z`` is added, ``z`` standard
    normal, so that the level behind the step is ``sigma'``:

        sigma_up   = min(sigma', eta * sqrt(sigma'^2 * (sigma^2 - sigma'^2) / sigma^2))
        sigma_down = sqrt(sigma'^2 - sigma_up^2),        n = s_noise * sigma_up

    At ``sigma' = 0`` both are 0 (a plain Euler step to 0); ``eta = 0`` gives ``(sigma', 0)`` exactly, the Euler sampler."""
    sig = _sigma_list(sigmas)
    eta, s_noise = _noise_parameters(eta, s_noise)
    out = []
    for s, s_next in zip(sig[:-1], sig[1:]):
        if s_next == 0.0 or eta == 0.0:
            out.append((s_next, 0.0))
            continue
        up = min(s_next, eta * math.sqrt(s_next * s_next * (s * s - s_next * s_next) / (s * s)))
        out.append((math.sqrt(s_next * s_next - up * up), s_noise * up))
    return out


def dpmpp_2m_sde_coefficients(sigmas: Sequence[float], eta: float = 1.0,
                              s_noise: float = 1.0) -> list[tuple[float, float, float, float, float]]:
    """One ``(a, b, c1, c2, n)`` per step of DPM-Solver++(2M) SDE: ``x' = a*x + b*(c1*D - c2*D_prev) + n*z``.

    k-diffusion's ``sample_dpmpp_2m_sde``, ``solver_type="midpoint"``, written in sigma with ``h = ln(sigma/sigma')``:

        a = (sigma'/sigma) * exp(-eta*h),    b = -expm1(-(1 + eta)*h),    n = s_noise * sigma' * sqrt(-expm1(-2*eta*h))

    ``c2 = h / (2*h_last)`` and ``c1 = 1 + c2`` as for ``dpmpp_2m_coefficients``; ``c1 = 1, c2 = 0`` at step 0 and at
    ``sigma' = 0``, where the tuple is ``(0, 1, 1, 0, 0)``: ``x' = D``.  The variance bookkeeping is
    ``a^2*sigma^2 + (n/s_noise)^2 = sigma'^2``.  With ``eta == 0`` the tuples are ``dpmpp_2m_coefficients``' own with
    ``n = 0``, so the kernels get the same fp32 constants.

    What differs from k-diffusion: there ``z`` comes from a Brownian tree over sigma (``BrownianTreeNoiseSampler``), so that
    the noise of a sigma interval is consistent across step lists.  Here ``z`` is drawn independently at every step
    (csrc/noise.h: a function of the video's seed, the step index and the element).  On a fixed step list the increments of a
    Brownian motion over disjoint intervals are independent too, so the samples have the same distribution; they are not
    the same numbers, and changing the number of steps changes the noise."""
    sig = _sigma_list(sigmas)
    eta, s_noise = _noise_parameters(eta, s_noise)
    if eta == 0.0:
        return [c + (0.0,) for c in dpmpp_2m_coefficients(sig)]
    out = []
    for i in range(len(sig) - 1):
        s, s_next = sig[i], sig[i + 1]
        if s_next == 0.0:
            out.append((0.0, 1.0, 1.0, 0.0, 0.0))
            continue
        h = math.log(s / s_next)
        c2 = h / (2.0 * math.log(sig[i - 1] / s)) if i > 0 else 0.0
        out.append(((s_next / s) * math.exp(-eta * h), -math.expm1(-(1.0 + eta) * h), 1.0 + c2, c2,
                    s_noise * s_next * math.sqrt(-math.expm1(-2.0 * eta * h))))
    return out
