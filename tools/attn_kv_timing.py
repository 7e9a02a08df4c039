#!/usr/bin/env python3
"""Spatial self-attention over pooled keys and values (sp_kv_pool_f16 + sp_attn_spatial_kv_f16, csrc/attention_kv.hip)
against the route the engine takes today on the same fused QKV buffer: sp_attn_spatial_long_f16 at level 0 of a two-video
forward (28 frames x 9,216 tokens, 5 heads) and sp_attn_spatial_f16 at level 1 (28 x 2,304, 10 heads), at factor 2 and 4; one
process, arms alternating, events around single calls.  Then whole forwards through tools/ab_forward.py in a child
process.  Writes profiles/attn_kv_timing.txt.   usage: attn_kv_timing.py [--reps 7] [--no-forwards]"""
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


def level(name, inst, h, w, heads, reps, lines):
    hw, c = h * w, heads * 64
    qkv = torch.randn(inst * hw, 3 * c, generator=torch.Generator().manual_seed(hw)).half().to(DEV)
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
    o_base, o_kv = (torch.empty(inst * hw, c, dtype=torch.float16, device=DEV) for _ in range(2))
    ld = dict(ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c)
    if hw >= 8192:                                          # the engine's default route at this length
        ws = torch.empty(ops.attn_long_ws_bytes(inst, hw, heads), dtype=torch.uint8, device=DEV)
        base_name, base = "sp_attn_spatial_long_f16", lambda: ops.attn_spatial_long(q, k, v, o_base, ws, **ld, batch=inst, seq=hw, heads=heads)
    else:
        base_name, base = "sp_attn_spatial_f16", lambda: ops.attn_spatial(q, k, v, o_base, **ld, batch=inst, seq=hw, heads=heads)
    lines.append(f"{name}: {inst} frames x {hw} tokens ({h} x {w}), {heads} heads")
    for f in (2, 4):
        rows = inst * hw // (f * f)
        kp, vp = (torch.empty(rows, c, dtype=torch.float16, device=DEV) for _ in range(2))

        def pool():
            ops.kv_pool(k, v, kp, vp, ldk=3 * c, ldv=3 * c, ldkp=c, ldvp=c, n_img=inst, h=h, w=w, c=c, factor=f)

        def attn():
            ops.attn_spatial_kv(q, kp, vp, o_kv, ldq=3 * c, ldk=c, ldv=c, ldo=c, batch=inst, seq_q=hw, seq_kv=hw // (f * f), heads=heads)

        def both():
            pool(); attn()

        t = {"base": [], "pool": [], "attn": [], "both": []}
        for _ in range(3):                                   # arms alternate
            t["base"] += timed(base, reps)
            t["pool"] += timed(pool, reps)
            t["attn"] += timed(attn, reps)
            t["both"] += timed(both, reps)
        med = {n: statistics.median(x) for n, x in t.items()}
        fl = 4.0 * inst * heads * hw * 64
        pool_bytes = 4.0 * inst * hw * c * (1 + 1 / (f * f))
        for n, label, extra in (("base", base_name, f"{fl * hw / med['base'] / 1e9:7.1f} TFLOP/s"),
                                ("pool", f"sp_kv_pool_f16 f={f}", f"{pool_bytes / med['pool'] / 1e6:7.0f} GB/s"),
                                ("attn", f"sp_attn_spatial_kv_f16 f={f}", f"{fl * hw / (f * f) / med['attn'] / 1e9:7.1f} TFLOP/s"),
                                ("both", f"pool + attention f={f}", "")):
            lines.append(f"  {label:30s} median {med[n]:8.3f} ms (min {min(t[n]):.3f}, max {max(t[n]):.3f}, n={len(t[n])})  {extra}")
        lines.append(f"  f={f}: {base_name} / (pool + attention) = {med['base'] / med['both']:.2f}x; the outputs differ by rel-L2 "
                     f"{float((o_kv.float() - o_base.float()).norm() / o_base.float().norm()):.2e} on Gaussian operands (an approximation)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-forwards", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_kv_timing.txt"))
    a = ap.parse_args()
    lines = [f"tools/attn_kv_timing.py on {torch.cuda.get_device_name(0)}: events around single calls, arms alternating in one "
             f"process, Gaussian operands in one fused QKV buffer (FLOP = 4 seq_q seq_kv 64 per frame and head; pooling bytes = K and V "
             f"read once, Kp and Vp written once; repeated calls on the same buffers, so the pooling rate is a cache rate, not HBM's)"]
    level("level 0", 28, 72, 128, 5, a.reps, lines)
    level("level 1", 28, 36, 64, 10, a.reps, lines)
    if not a.no_forwards:
        torch.cuda.synchronize()
        lines.append("whole forwards (tools/ab_forward.py base unet:kv_downsample=2 unet:kv_downsample=4; a child process):")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_forward.py"), "base", "unet:kv_downsample=2",
                              "unet:kv_downsample=4"], capture_output=True, text=True, check=True).stdout
        lines += ["  " + ln for ln in out.splitlines() if "ms per video" in ln]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
