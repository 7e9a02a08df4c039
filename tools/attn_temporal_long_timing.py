#!/usr/bin/env python3
"""Temporal self-attention for long clips (sp_attn_temporal_long_f16, csrc/attention_temporal_long.hip) at 48, 64, 96 and 128
frames and, in the same run, sp_attn_temporal_f16 at 25 and 32 frames, at the level-0 and level-1 shapes of one video (9,216
tokens x 5 heads, 2,304 x 10) on a fused QKV buffer; one process, arms alternating, events around single calls, medians with
their spread, microseconds and microseconds per problems x frames^2 (the two kernels per unit of work).  Then one whole forward
of the tiny configuration at 48 frames.  Nothing is asserted: the file records what was seen.
Writes profiles/attn_temporal_long_timing.txt.   usage: attn_temporal_long_timing.py [--reps 7]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import vdpp_amd  # noqa: F401
from vdpp_amd.hip import ops

DEV = "cuda:0"
ARMS = (25, 32, 48, 64, 96, 128)


def timed(fn, reps):
    """Milliseconds of `reps` single calls (events around each), after two warm-up calls."""
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def level(name, hw, heads, reps, lines):
    c = heads * 64
    qkv = torch.randn(max(ARMS) * hw, 3 * c, generator=torch.Generator(DEV).manual_seed(hw), device=DEV, dtype=torch.float16)
    o = torch.empty(max(ARMS) * hw, c, dtype=torch.float16, device=DEV)
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]

    def arm(frames):
        call = ops.attn_temporal_long if frames > 32 else ops.attn_temporal
        return lambda: call(q, k, v, o, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, batch=1, frames=frames, hw=hw, heads=heads)

    t = {f: [] for f in ARMS}
    for _ in range(3):                                       # arms alternate
        for f in ARMS:
            t[f] += timed(arm(f), reps)
    lines.append(f"{name}: one video, {hw} tokens per frame, {heads} heads = {hw * heads} problems")
    for f in ARMS:
        med, units = statistics.median(t[f]) * 1e3, hw * heads * f * f
        lines.append(f"  {'sp_attn_temporal_long_f16' if f > 32 else 'sp_attn_temporal_f16':26s} {f:4d} frames  median {med:9.1f} us "
                     f"(min {min(t[f]) * 1e3:.1f}, max {max(t[f]) * 1e3:.1f}, n={len(t[f])})  {med / units * 1e6:7.3f} us per 10^6 problems x frames^2  "
                     f"{8.0 * f * hw * c / med / 1e3:6.0f} GB/s of Q, K, V, O")


def tiny_forward(reps, lines):
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict
    cfg = UNetConfig.tiny(64)
    hip = SVDUNetHIP(cfg, random_state_dict(cfg, seed=3, dtype=torch.float16), DEV)
    g = torch.Generator().manual_seed(11)
    ctx, ids = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half().to(DEV), torch.tensor([[5.0, 127.0, 0.02]]).half().to(DEV)
    for frames in (25, 48):
        sample = torch.randn(1, frames, 8, 16, 16, generator=g).half().to(DEV)
        t = timed(lambda: hip(sample, 1.63777, ctx, ids), reps)
        lines.append(f"  tiny configuration, one forward at {frames} frames of 16 x 16: median {statistics.median(t):.2f} ms "
                     f"(min {min(t):.2f}, max {max(t):.2f}, n={len(t)}; launch-bound at this size)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_temporal_long_timing.txt"))
    a = ap.parse_args()
    lines = [f"tools/attn_temporal_long_timing.py on {torch.cuda.get_device_name(0)}: events around single calls, arms alternating in "
             f"one process, Gaussian operands in one fused QKV buffer; a unit of work is one (problem, query frame, key frame) pair; "
             f"bytes = Q, K, V read once and O written once.  No speed is promised or asserted; nothing was tuned to these numbers."]
    level("level 0", 9216, 5, a.reps, lines)
    level("level 1", 2304, 10, a.reps, lines)
    lines.append("whole forwards (SVDUNetHIP, UNetConfig.tiny(64), random weights):")
    tiny_forward(a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
