"""Host plan of a long video denoised as overlapping frame windows (temporal co-denoising).

``frames_total`` frames are cut into ``n_win = (frames_total - window)/stride + 1`` windows of ``window`` frames -- the frame
count the model was conditioned for -- window ``k`` covering global frames ``k*stride .. k*stride + window - 1``.  Every step
evaluates the UNet on each window and blends the predictions per global frame with the normalised weights

    wn[k][p] = alpha(p) / sum over the windows k' covering f = k*stride + p of alpha(f - k'*stride)

``alpha(p) = min(p + 1, window - p)`` ("triangle": a window counts most at its centre) or 1 ("uniform").  The table is made in
fp64 and handed to the kernels (``sp_euler_step_windows_f16`` / ``sp_dpmpp2m_step_windows_f16``) as fp32 ``[n_win][window]``.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

WEIGHTS = ("triangle", "uniform")


@dataclass(frozen=True, eq=False)
class WindowPlan:
    frames_total: int
    window: int
    stride: int
    starts: tuple            # first global frame of every window
    weights: np.ndarray      # fp32 [n_win][window], sums to 1 over the windows covering each global frame
    profile: str

    @property
    def n_win(self) -> int:
        return len(self.starts)

    def coverage(self) -> np.ndarray:
        """How many windows cover each global frame (at most ``ceil(window/stride)``)."""
        count = np.zeros(self.frames_total, dtype=np.int64)
        for s in self.starts:
            count[s:s + self.window] += 1
        return count


def legal_totals(frames_total: int, window: int, stride: int) -> tuple:
    """The legal totals nearest to ``frames_total`` from below and above (the same number twice where it is legal)."""
    if frames_total <= window:
        return window, window
    below = window + (frames_total - window) // stride * stride
    return below, below if below == frames_total else below + stride


def profile(window: int, weights: str = "triangle") -> np.ndarray:
    """``alpha`` over the positions of a window, fp64."""
    if weights not in WEIGHTS:
        raise ValueError(f"window_weights must be one of {WEIGHTS}; got {weights!r}")
    p = np.arange(window, dtype=np.float64)
    return np.minimum(p + 1.0, window - p) if weights == "triangle" else np.ones(window, dtype=np.float64)


def plan(frames_total: int, window: int, stride: int, weights: str = "triangle") -> WindowPlan:
    frames_total, window, stride = int(frames_total), int(window), int(stride)
    what = f"window plan (frames_total={frames_total}, window={window}, stride={stride})"
    if window < 1 or frames_total < window:
        raise ValueError(f"{what}: frames_total must be at least window, and window at least 1")
    if not 1 <= stride <= window:
        raise ValueError(f"{what}: stride must be from 1 to window (a larger stride leaves frames that no window covers)")
    if (frames_total - window) % stride:
        lo, hi = legal_totals(frames_total, window, stride)
        raise ValueError(f"{what}: frames_total is not window plus a whole number of strides; the nearest legal totals are "
                         f"{lo} and {hi}")
    alpha = profile(window, weights)
    starts = tuple(range(0, frames_total - window + 1, stride))
    total = np.zeros(frames_total, dtype=np.float64)
    for s in starts:
        total[s:s + window] += alpha
    table = np.stack([alpha / total[s:s + window] for s in starts]).astype(np.float32)
    return WindowPlan(frames_total=frames_total, window=window, stride=stride, starts=starts, weights=table, profile=weights)


def noise_shape(batch: int, frames_total: int, height: int, width: int, window: int, stride: int) -> tuple:
    """The shape (B, 4, F_total, H/8, W/8) of the initial noise of a windowed run, after checking the triple."""
    plan(frames_total, window, stride)
    if height % 8 or width % 8:
        raise ValueError(f"height={height} and width={width} must be multiples of 8")
    return (int(batch), 4, int(frames_total), height // 8, width // 8)
