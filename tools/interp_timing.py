#!/usr/bin/env python3
"""What frames between the frames cost, per video of 14 frames of 576 x 1024 on the device (profiles/interp_timing.txt):

  * sp_interp_motion_u8 (luma, search, median) and sp_interp_compensate_u8, each on its own, for the first round (14 frames
    -> 27) and the second (27 -> 53), at search ranges 8, 16 and 24;
  * FrameInterpolator as a whole at factor 2 and factor 4 (device events around the call, and a host clock around a call
    that ends synchronised);
  * beside them the temporal-VAE decode of the same video, from profiles/image_io_timing.txt (the stage this one follows).

Input: a smooth two-sinusoid colour field that moves from frame to frame plus sigma = 8 noise (the field of the codec
timings); the search is exhaustive, so its time does not depend on the picture.  NWARM warm-up rounds, then the median,
minimum and maximum of NREP rounds.  A record, not a pass condition: nothing here was tuned to a number.
usage: interp_timing.py [output file]   (environment: NREP=10 NWARM=2; default output profiles/interp_timing.txt)"""
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import vdpp_amd  # noqa
from vdpp_amd.hip import ops
from vdpp_amd.models.image_io import FrameInterpolator

NREP, NWARM = max(10, int(os.environ.get("NREP", 10))), int(os.environ.get("NWARM", 2))
F, H, W = 14, 576, 1024
RANGES = (8, 16, 24)
PENALTY = 4
dev = torch.device("cuda:0")


def scene(seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((F, H, W, 3))
    for f in range(F):
        for c in range(3):
            out[f, :, :, c] = (128 + 70 * np.sin(2 * np.pi * (x / (37.0 + 9 * c) + 0.13 * f))
                               + 45 * np.sin(2 * np.pi * (y / (23.0 + 5 * c) + x / 91.0 - 0.07 * f * (c + 1))))
    return np.clip(np.rint(out + rng.normal(0, 8, out.shape)), 0, 255).astype(np.uint8)


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def med(t):
    return sorted(t)[len(t) // 2]


def line(name, t):
    return f"  {name}: median {med(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f})"


def decode_ms():
    """The median of decode_latents_uint8 in profiles/image_io_timing.txt, or None."""
    try:
        with open(os.path.join(ROOT, "profiles", "image_io_timing.txt")) as fh:
            m = re.search(r"^decode_latents_uint8 .*?median ([0-9.]+) ms", fh.read(), re.M)
        return float(m.group(1)) if m else None
    except OSError:
        return None


def main():
    frames = torch.from_numpy(scene()).to(dev)
    lines = [f"Frame interpolation of one video, {F} frames of {H}x{W} (python tools/interp_timing.py, one MI355X).",
             f"device: {torch.cuda.get_device_name(0)}; penalty {PENALTY}; {NWARM} warm-up rounds, then {NREP} timed rounds per line.",
             "Device events around the entry points and around FrameInterpolator; the host clock around a call that ends",
             "synchronised.  A record, not a pass condition.", ""]
    decode = decode_ms()
    whole = {}
    for R in RANGES:
        t = {}
        rounds = []
        src = frames
        for rnd in range(2):
            n = src.shape[0]
            ws = torch.empty(ops.interp_ws_bytes(n, H, W, R), dtype=torch.uint8, device=dev)
            vec = torch.empty((n - 1, H // 8, W // 8, 2), dtype=torch.int16, device=dev)
            out = torch.empty((2 * n - 1, H, W, 3), dtype=torch.uint8, device=dev)
            rounds.append((src, ws, vec, out))
            ops.interp_motion(src, vec, ws, search_range=R, penalty=PENALTY)
            src = ops.interp_compensate(src, vec, out)
        interp = {f: FrameInterpolator(dev, H, W, factor=f, search_range=R, penalty=PENALTY) for f in (2, 4)}
        for it in range(NWARM + NREP):
            r_ = {}
            for rnd, (src, ws, vec, out) in enumerate(rounds):
                r_[f"motion{rnd}"], _ = device_ms(lambda: ops.interp_motion(src, vec, ws, search_range=R, penalty=PENALTY))
                r_[f"compensate{rnd}"], _ = device_ms(lambda: ops.interp_compensate(src, vec, out))
            for f in (2, 4):
                r_[f"device{f}"], got = device_ms(lambda: interp[f](frames))
                r_[f"host{f}"], _ = host_ms(lambda: interp[f](frames))
                assert got.shape[0] == (F - 1) * f + 1
            if it >= NWARM:
                for k, v in r_.items():
                    t.setdefault(k, []).append(v)
        assert torch.equal(interp[2](frames), rounds[0][3]) and torch.equal(interp[4](frames), rounds[1][3])
        cand = (2 * R + 1) ** 2
        lines.append(f"search range {R} ({cand} candidates per block, {(H // 8) * (W // 8)} blocks per pair):")
        for rnd, (src, _, _, _) in enumerate(rounds):
            n = src.shape[0]
            diffs = (n - 1) * (H // 8) * (W // 8) * cand * 256
            m = med(t[f"motion{rnd}"])
            lines.append(line(f"round {rnd + 1}, sp_interp_motion_u8, {n} frames, {n - 1} pairs", t[f"motion{rnd}"])
                         + f"; {diffs / 1e9:.1f} G byte differences, {diffs / m / 1e9:.2f} T/s")
            lines.append(line(f"round {rnd + 1}, sp_interp_compensate_u8, {n} -> {2 * n - 1} frames", t[f"compensate{rnd}"]))
        for f in (2, 4):
            lines.append(line(f"FrameInterpolator factor {f}, {F} -> {(F - 1) * f + 1} frames (device events)", t[f"device{f}"]))
            lines.append(line(f"FrameInterpolator factor {f} (host clock, synchronised)", t[f"host{f}"]))
            whole[(R, f)] = med(t[f"device{f}"])
        lines.append("")
    if decode is not None:
        lines.append(f"decode_latents_uint8 of the same video (profiles/image_io_timing.txt): median {decode:.3f} ms")
        for (R, f), m in whole.items():
            lines.append(f"  range {R:>2}, factor {f}: {m:.3f} ms, {100.0 * m / decode:.2f} % of the decode"
                         + ("  (SLOWER than the decode it follows)" if m > decode else ""))
    else:
        lines.append("profiles/image_io_timing.txt was not found: no decode time to compare with")
    text = "\n".join(lines) + "\n"
    print(text)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "interp_timing.txt")
    with open(path, "w") as fh:
        fh.write(text)


with torch.no_grad():
    main()
