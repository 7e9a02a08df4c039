"""Host plan of a large frame denoised as overlapping spatial tiles (spatial co-denoising).

Units are latent cells.  Per axis the rule of ``window_plan.plan``: a total ``T`` is cut into ``n = (T - t)/s + 1`` tiles of
``t`` cells -- the size the model was trained at -- tile ``k`` covering cells ``k*s .. k*s + t - 1``
(``1 <= s <= t <= T``, ``(T - t) % s == 0``).  A patch is one frame window times one tile, patch
``k = (kf*n_ty + ky)*n_tx + kx``; every step evaluates the UNet on each patch and blends the predictions per element with

    w_k = wf[kf][f - kf*sf] * wy[ky][y - ky*sy] * wx[kx][x - kx*sx]

The profile of a patch is the product of the per-axis profiles, so its normaliser -- the sum over the covering patches -- is
the product of the per-axis normalisers and the weights stay separable: the kernels (``sp_euler_step_tiles_f16`` /
``sp_dpmpp2m_step_tiles_f16``) get the three small fp32 tables, each made in fp64 by ``window_plan.plan``, and never a
per-pixel table.  Without frame windows the frame plan is one window that is the whole video (``wf`` all 1.0).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import window_plan
from .window_plan import WEIGHTS, WindowPlan, legal_totals, profile  # noqa: F401  (the same rule, profiles and error texts)


@dataclass(frozen=True, eq=False)
class TilePlan:
    y: WindowPlan            # along the rows: total H, tile th, stride sy
    x: WindowPlan            # along the columns: total W, tile tw, stride sx
    frames: WindowPlan       # the frame plan; one window that is the whole video where window_stride is not set
    profile: str

    @property
    def n_ty(self) -> int:
        return self.y.n_win

    @property
    def n_tx(self) -> int:
        return self.x.n_win

    @property
    def n_patch(self) -> int:
        return self.frames.n_win * self.n_ty * self.n_tx

    @property
    def tile(self) -> tuple:
        return self.y.window, self.x.window

    @property
    def wf(self) -> np.ndarray:
        return self.frames.weights

    @property
    def wy(self) -> np.ndarray:
        return self.y.weights

    @property
    def wx(self) -> np.ndarray:
        return self.x.weights

    def patch_index(self, kf: int, ky: int, kx: int) -> int:
        return (kf * self.n_ty + ky) * self.n_tx + kx

    def patches(self) -> list:
        """``(kf, ky, kx, first frame, first row, first column)`` of every patch, in the order of the eps buffer."""
        return [(kf, ky, kx, f0, y0, x0) for kf, f0 in enumerate(self.frames.starts) for ky, y0 in enumerate(self.y.starts)
                for kx, x0 in enumerate(self.x.starts)]

    def coverage(self) -> np.ndarray:
        """How many patches cover each element ``[F_total][H][W]`` (at most the product of ``ceil(t/s)`` over the axes)."""
        return (self.frames.coverage()[:, None, None] * self.y.coverage()[None, :, None] * self.x.coverage()[None, None, :])


def _axis(name: str, total: int, tile: int, stride: int, weights: str) -> WindowPlan:
    total, tile, stride = int(total), int(tile), int(stride)
    what = f"tile plan, {name} (total={total}, tile={tile}, stride={stride})"
    if tile < 1 or total < tile:
        raise ValueError(f"{what}: total must be at least tile, and tile at least 1")
    if not 1 <= stride <= tile:
        raise ValueError(f"{what}: stride must be from 1 to tile (a larger stride leaves cells that no tile covers)")
    if (total - tile) % stride:
        lo, hi = legal_totals(total, tile, stride)
        raise ValueError(f"{what}: total is not tile plus a whole number of strides; the nearest legal totals are {lo} and {hi}")
    return window_plan.plan(total, tile, stride, weights)


def plan(height: int, width: int, tile_size, tile_stride, weights: str = "triangle", *, frames_total: int = 1,
         window: int | None = None, window_stride: int | None = None, window_weights: str | None = None) -> TilePlan:
    """The plan of an ``height x width`` latent cut into tiles ``tile_size = (th, tw)``, ``tile_stride = (sy, sx)`` apart, times
    the frame windows ``(frames_total, window, window_stride)`` (``window=None``: one window that is the whole video)."""
    if weights not in WEIGHTS:
        raise ValueError(f"tile_weights must be one of {WEIGHTS}; got {weights!r}")
    (th, tw), (sy, sx) = _pair("tile_size", tile_size), _pair("tile_stride", tile_stride)
    ay = _axis("y", height, th, sy, weights)
    ax = _axis("x", width, tw, sx, weights)
    if window is None:
        window = window_stride = int(frames_total)
    frames = window_plan.plan(frames_total, window, window if window_stride is None else window_stride,
                              weights if window_weights is None else window_weights)
    return TilePlan(y=ay, x=ax, frames=frames, profile=weights)


def _pair(name: str, value) -> tuple:
    try:
        a, b = value
        return int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a pair of latent cell counts (y, x); got {value!r}") from None


def noise_shape(batch: int, frames_total: int, height: int, width: int, tile_height: int, tile_width: int, stride_y: int,
                stride_x: int) -> tuple:
    """The shape (B, 4, F, H/8, W/8) of the initial noise of a tiled run, after checking both triples; all sizes in pixels."""
    for name, v in (("height", height), ("width", width), ("tile height", tile_height), ("tile width", tile_width),
                    ("tile stride y", stride_y), ("tile stride x", stride_x)):
        if int(v) % 8:
            raise ValueError(f"{name}={v} must be a multiple of 8")
    plan(height // 8, width // 8, (tile_height // 8, tile_width // 8), (stride_y // 8, stride_x // 8))
    return (int(batch), 4, int(frames_total), height // 8, width // 8)
