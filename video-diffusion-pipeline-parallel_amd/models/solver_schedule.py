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

SAMPLERS = ("euler", "dpmpp_2m")


def dpmpp_2m_coefficients(sigmas: Sequence[float]) -> list[tuple[float, float, float, float]]:
    """One ``(a, b, c1, c2)`` per step for the sigma table ``sigmas`` (``N + 1`` entries, decreasing, the last may be 0).

    ``a = sigma'/sigma``, ``b = 1 - a``; ``c2 = h / (2*h_last)`` with ``h = ln(sigma/sigma')``, ``h_last =
    ln(sigma_prev/sigma)`` and ``c1 = 1 + c2``, except ``c1 = 1, c2 = 0`` at step 0 and where ``sigma' = 0``."""
    sig = [float(s) for s in (sigmas.tolist() if hasattr(sigmas, "tolist") else sigmas)]
    if len(sig) < 2:
        raise ValueError("a sigma table has at least two entries (one step)")
    for i in range(len(sig) - 1):
        if not (sig[i] > 0.0 and 0.0 <= sig[i + 1] < sig[i]):
            raise ValueError(f"sigmas must be positive and strictly decreasing (the last may be 0); got {sig[i]!r} -> "
                             f"{sig[i + 1]!r} at step {i}")
    out = []
    for i in range(len(sig) - 1):
        s, s_next = sig[i], sig[i + 1]
        a = s_next / s
        c2 = 0.0
        if i > 0 and s_next > 0.0:
            c2 = math.log(s / s_next) / (2.0 * math.log(sig[i - 1] / s))
        out.append((a, 1.0 - a, 1.0 + c2, c2))
    return out
