"""The frame interpolator's numpy statement: bilateral block motion search, a 3x3 vector median and overlapped
compensation, all in integers.  ``csrc/interp.hip`` must equal it bit for bit (tests/test_interp_gpu.py); its own
properties, and the planted mistakes below, are in tests/test_interp_cpu.py.

  luma      Y = (77 R + 150 G + 29 B + 128) >> 8
  search    per pair (A, B) and 8x8 block (by, bx) of the midpoint's grid, over all v = (vy, vx) in [-R, R]^2:
              cost(v) = sum_q |YA[clamp(q - v)] - YB[clamp(q + v)]| + lam (|vy| + |vx|)
            q over the 16x16 window with origin (8 by - 4, 8 bx - 4), unclamped; clamp acts on the displaced coordinate,
            per axis, to the image.  key(v) = cost * 4096 + ((vy + R) (2R + 1) + (vx + R)); the raw vector has the least key.
  median    component-wise 5th smallest of the 3x3 neighbourhood of raw vectors, block coordinates clamped to the grid
  blend     pixel (y, x): ty = y + 4, by0 = (ty >> 3) - 1, wy1 = 2 (ty & 7) + 1, wy0 = 16 - wy1, likewise x; the four blocks
            (by0 + {0, 1}, bx0 + {0, 1}) clamped to the grid, weights wy wx (sum 256):
              out_c = (sum_k w_k (A_c[clamp(p - v_k)] + B_c[clamp(p + v_k)]) + 256) >> 9

``mutant`` names one planted mistake (MUTANTS); None is the statement itself.
"""

from __future__ import annotations

import numpy as np

MUTANTS = ("ties_last", "origin_8by", "clamp_window_first", "same_sign", "index_swapped", "no_penalty", "median_raw",
           "median_4th", "weight_no_plus_1", "no_rounding", "luma_no_128")


def check_args(frames, R: int, lam: int) -> np.ndarray:
    a = np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"frames must be (N, H, W, 3) uint8; got {a.dtype} {a.shape}")
    n, h, w, _ = a.shape
    if n < 2 or h % 8 or w % 8 or h < 16 or w < 16:
        raise ValueError(f"frames must be at least 2 of a size that is a multiple of 8 and at least 16; got {a.shape}")
    if not 1 <= R <= 24 or not 0 <= lam <= 255:
        raise ValueError(f"R must be 1..24 and lam 0..255; got {R}, {lam}")
    return a


def luma(frame: np.ndarray, mutant=None) -> np.ndarray:
    f = frame.astype(np.int32)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + (0 if mutant == "luma_no_128" else 128)) >> 8


def _displaced(plane: np.ndarray, q0: int, v: tuple[int, int], sign: int, clamp_first: bool) -> np.ndarray:
    """plane[clamp(q + sign v)] for q over [q0, q0 + H + 8) x [q0, q0 + W + 8)."""
    h, w = plane.shape
    qy, qx = np.arange(q0, q0 + h + 8), np.arange(q0, q0 + w + 8)
    if clamp_first:
        qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
    return plane[np.clip(qy + sign * v[0], 0, h - 1)[:, None], np.clip(qx + sign * v[1], 0, w - 1)[None, :]]


def search(ya: np.ndarray, yb: np.ndarray, R: int, lam: int, mutant=None) -> np.ndarray:
    """Raw vectors (H/8, W/8, 2) int16 in (vy, vx) order."""
    h, w = ya.shape
    bh, bw = h // 8, w // 8
    q0 = 0 if mutant == "origin_8by" else -4
    side = 2 * R + 1
    best = np.full((bh, bw), np.iinfo(np.int64).max, np.int64)
    for vy in range(-R, R + 1):
        for vx in range(-R, R + 1):
            da = _displaced(ya, q0, (vy, vx), -1, mutant == "clamp_window_first")
            db = _displaced(yb, q0, (vy, vx), -1 if mutant == "same_sign" else 1, mutant == "clamp_window_first")
            cells = np.abs(da - db).reshape(bh + 1, 8, bw + 1, 8).sum(axis=(1, 3), dtype=np.int64)
            cost = cells[:-1, :-1] + cells[1:, :-1] + cells[:-1, 1:] + cells[1:, 1:]
            if mutant != "no_penalty":
                cost = cost + lam * (abs(vy) + abs(vx))
            idx = (vx + R) * side + (vy + R) if mutant == "index_swapped" else (vy + R) * side + (vx + R)
            best = np.minimum(best, cost * 4096 + (4095 - idx if mutant == "ties_last" else idx))
    idx = best & 4095
    if mutant == "ties_last":
        idx = 4095 - idx
    first, second = idx // side - R, idx % side - R
    if mutant == "index_swapped":
        first, second = second, first
    return np.stack([first, second], axis=-1).astype(np.int16)


def median(raw: np.ndarray, mutant=None) -> np.ndarray:
    if mutant == "median_raw":
        return raw.copy()
    bh, bw, _ = raw.shape
    ys, xs = np.arange(bh), np.arange(bw)
    nine = [raw[np.clip(ys + dy, 0, bh - 1)[:, None], np.clip(xs + dx, 0, bw - 1)[None, :]]
            for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return np.sort(np.stack(nine), axis=0)[3 if mutant == "median_4th" else 4]


def compensate(a: np.ndarray, b: np.ndarray, vectors: np.ndarray, mutant=None) -> np.ndarray:
    h, w, _ = a.shape
    bh, bw = h // 8, w // 8
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    ty, tx = ys + 4, xs + 4
    one = 0 if mutant == "weight_no_plus_1" else 1
    wy1, wx1 = 2 * (ty & 7) + one, 2 * (tx & 7) + one
    acc = np.zeros((h, w, 3), np.int32)
    for dy, wy in ((0, 16 - wy1), (1, wy1)):
        for dx, wx in ((0, 16 - wx1), (1, wx1)):
            v = vectors[np.clip((ty >> 3) - 1 + dy, 0, bh - 1), np.clip((tx >> 3) - 1 + dx, 0, bw - 1)].astype(np.int32)
            vy, vx = v[..., 0], v[..., 1]
            pa = a[np.clip(ys - vy, 0, h - 1), np.clip(xs - vx, 0, w - 1)].astype(np.int32)
            pb = b[np.clip(ys + vy, 0, h - 1), np.clip(xs + vx, 0, w - 1)].astype(np.int32)
            acc += (wy * wx)[..., None] * (pa + pb)
    return ((acc + (0 if mutant == "no_rounding" else 256)) >> 9).astype(np.uint8)


def motion(frames, R: int = 16, lam: int = 4, mutant=None) -> tuple[np.ndarray, np.ndarray]:
    """``(vectors, raw_vectors)``, each (N - 1, H/8, W/8, 2) int16."""
    a = check_args(frames, R, lam)
    y = [luma(f, mutant) for f in a]
    raw = np.stack([search(y[i], y[i + 1], R, lam, mutant) for i in range(len(a) - 1)])
    return np.stack([median(r, mutant) for r in raw]), raw


def interpolate_round(frames, R: int = 16, lam: int = 4, mutant=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One round: ``(out (2N - 1, H, W, 3) uint8, vectors, raw_vectors)``."""
    a = check_args(frames, R, lam)
    vectors, raw = motion(a, R, lam, mutant)
    out = np.empty((2 * len(a) - 1,) + a.shape[1:], np.uint8)
    out[0::2] = a
    for i in range(len(a) - 1):
        out[2 * i + 1] = compensate(a[i], a[i + 1], vectors[i], mutant)
    return out, vectors, raw


def interpolate(frames, factor: int = 2, R: int = 16, lam: int = 4) -> np.ndarray:
    """((N - 1) factor + 1, H, W, 3) uint8; factor 4 is two rounds."""
    if factor not in (1, 2, 4):
        raise ValueError("factor must be 1, 2 or 4")
    a = check_args(frames, R, lam)
    while factor > 1:
        a, factor = interpolate_round(a, R, lam)[0], factor // 2
    return a


def rounded_average(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return ((a.astype(np.int32) + b + 1) >> 1).astype(np.uint8)


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


# ---- test pictures -----------------------------------------------------------------------------------------------------
def smoothed_noise(rng, h: int, w: int, passes: int = 3) -> np.ndarray:
    """(h, w, 3) uint8: white noise under `passes` 3x3 box filters (wrapping), stretched back to the full range."""
    x = rng.random((h, w, 3))
    for _ in range(passes):
        x = sum(np.roll(np.roll(x, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    x = (x - x.min()) / (x.max() - x.min())
    return (x * 255.0 + 0.5).astype(np.uint8)


def crop_at(picture: np.ndarray, h: int, w: int, offset: tuple[int, int]) -> np.ndarray:
    """The crop whose content is moved by `offset` from the centred one."""
    oy, ox = (picture.shape[0] - h) // 2, (picture.shape[1] - w) // 2
    return picture[oy - offset[0]: oy - offset[0] + h, ox - offset[1]: ox - offset[1] + w]


def moving_crop(picture: np.ndarray, h: int, w: int, u: tuple[int, int], n: int = 2) -> np.ndarray:
    """n frames (n, h, w, 3): frame i shows the picture's content moved by 2 u i, so the true midpoint of frames i and i + 1
    is ``crop_at(picture, h, w, (2 i + 1) u)``."""
    return np.stack([crop_at(picture, h, w, (2 * u[0] * i, 2 * u[1] * i)) for i in range(n)])


def two_object_scene(rng, h: int = 128, w: int = 192) -> np.ndarray:
    """Three frames half a frame time apart (A, the true middle, B): a static smoothed-noise background, a 48x48 patch that
    moves (8, 12) from A to B and a 40x56 patch that moves (-6, 4), each with a texture of its own."""
    back = smoothed_noise(rng, h, w)
    p1, p2 = smoothed_noise(rng, 48, 48, 2), smoothed_noise(rng, 40, 56, 2)
    frames = []
    for i in range(3):
        f = back.copy()
        y, x = 16 + 4 * i, 16 + 6 * i
        f[y:y + 48, x:x + 48] = p1
        y, x = 80 - 3 * i, 100 + 2 * i
        f[y:y + 40, x:x + 56] = p2
        frames.append(f)
    return np.stack(frames)
