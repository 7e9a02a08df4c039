#!/usr/bin/env python3
"""Spatial self-attention over a sliding window of 8 x 8 token tiles (sp_attn_spatial_window_f16, csrc/attention_window.hip)
at level 0 of a two-video forward (28 frames x 9,216 tokens = 72 x 128, 5 heads) against the route the engine takes today
on the same fused QKV buffer (sp_attn_spatial_long_f16) and against pooling + sp_attn_spatial_kv_f16 at factor 2; one
process, arms alternating, events around single calls.  Windows (3, 3), (5, 7) and (9, 17): the grid is 9 x 16 tiles and a
window is odd, so (9, 17) is the smallest that covers it -- effective (9, 16), full attention.  Then whole forwards
through tools/ab_forward.py in a child process.  Writes profiles/attn_window_timing.txt.
usage: attn_window_timing.py [--reps 10] [--no-forwards]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import vdpp_amd  # noqa: F401
from vdpp_amd.hip import ops

DEV = "cuda:0"
WINDOWS = [(3, 3), (5, 7), (9, 17)]


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


def level0(reps, lines, inst=28, h=72, w=128, heads=5):
    hw, c, gh, gw = h * w, heads * 64, h // 8, w // 8
    qkv = torch.randn(inst * hw, 3 * c, generator=torch.Generator().manual_seed(hw)).half().to(DEV)
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
    o_base, o_kv, o_win = (torch.empty(inst * hw, c, dtype=torch.float16, device=DEV) for _ in range(3))
    ld = dict(ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c)
    ws = torch.empty(ops.attn_long_ws_bytes(inst, hw, heads), dtype=torch.uint8, device=DEV)
    kp, vp = (torch.empty(inst * hw // 4, c, dtype=torch.float16, device=DEV) for _ in range(2))

    def pooled():
        ops.kv_pool(k, v, kp, vp, ldk=3 * c, ldv=3 * c, ldkp=c, ldvp=c, n_img=inst, h=h, w=w, c=c, factor=2)
        ops.attn_spatial_kv(q, kp, vp, o_kv, ldq=3 * c, ldk=c, ldv=c, ldo=c, batch=inst, seq_q=hw, seq_kv=hw // 4, heads=heads)

    arms = {"sp_attn_spatial_long_f16": (lambda: ops.attn_spatial_long(q, k, v, o_base, ws, **ld, batch=inst, seq=hw, heads=heads), hw),
            "pool + sp_attn_spatial_kv_f16 f=2": (pooled, hw // 4)}
    for wh, ww in WINDOWS:
        arms[f"sp_attn_spatial_window_f16 ({wh}, {ww})"] = (
            lambda wh=wh, ww=ww: ops.attn_spatial_window(q, k, v, o_win, **ld, batch=inst, h=h, w=w, heads=heads, wh=wh, ww=ww),
            64 * min(wh, gh) * min(ww, gw))
    t = {n: [] for n in arms}
    for _ in range(3):                                       # arms alternate
        for n, (fn, _) in arms.items():
            t[n] += timed(fn, reps)
    lines.append(f"level 0: {inst} frames x {hw} tokens ({h} x {w} = {gh} x {gw} tiles), {heads} heads")
    base = statistics.median(t["sp_attn_spatial_long_f16"])
    for n, (fn, keys) in arms.items():
        med = statistics.median(t[n])
        fn()
        torch.cuda.synchronize()
        out = o_base if n.startswith("sp_attn_spatial_long") else o_kv if n.startswith("pool") else o_win
        diff = float((out.float() - o_base.float()).norm() / o_base.float().norm())
        lines.append(f"  {n:38s} median {med:7.3f} ms (min {min(t[n]):.3f}, max {max(t[n]):.3f}, n={len(t[n])})  "
                     f"{4.0 * inst * heads * hw * keys * 64 / med / 1e9:6.1f} TFLOP/s of the scores computed   key share {keys / hw:.3f}   "
                     f"time share {med / base:.3f}   rel-L2 to the full output {diff:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-forwards", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_window_timing.txt"))
    a = ap.parse_args()
    lines = [f"tools/attn_window_timing.py on {torch.cuda.get_device_name(0)}: events around single calls, arms alternating in one "
             f"process, Gaussian operands in one fused QKV buffer (FLOP = 4 queries keys 64 per frame and head; key share = keys a "
             f"query meets / 9,216; time share = median / median of sp_attn_spatial_long_f16 in this run; on Gaussian operands a "
             f"window that is not the grid is a different function: the last column says how different, it is no error)"]
    level0(a.reps, lines)
    if not a.no_forwards:
        torch.cuda.synchronize()
        arms = ["base", "unet:spatial_window=5/7", "unet:spatial_window=3/3"]
        lines.append(f"whole forwards (tools/ab_forward.py {' '.join(arms)}; a child process):")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_forward.py")] + arms, capture_output=True, text=True,
                             check=True).stdout
        lines += ["  " + ln for ln in out.splitlines() if "ms per video" in ln]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
