#!/usr/bin/env python3
"""Fused single-head attention (sp_attn_wide_f16) against the composed core of the VAE mid block (Q.K^T into fp32 scores, row
softmax, V^T = W_v.X^T, P.V) on the same operands, one process, arms alternating; then the whole decode on both routes
with its peak memory.  Writes profiles/attn_wide_timing.txt.   usage: attn_wide_timing.py [--frames 14] [--reps 7]"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import vdpp_amd  # noqa: F401
from vdpp_amd.hip import ops
from vdpp_amd.models.vae_hip import (ATTN_LONG_FROM, TemporalDecoderHIP, VAEDecoderConfig, attn_row_blocks,
                                     random_state_dict)

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


def core(hw, c, reps, lines):
    g = torch.Generator().manual_seed(hw)
    x, q, k = (torch.randn(hw, c, generator=g).half().to(DEV) for _ in range(3))
    wv = (torch.randn(c, c, generator=g) / math.sqrt(c)).half().to(DEV)
    bv = torch.zeros(c, device=DEV)
    v = (x.float() @ wv.float().t()).half()
    o_f, o_c = torch.empty(hw, c, dtype=torch.float16, device=DEV), torch.empty(hw, c, dtype=torch.float16, device=DEV)
    vt = torch.empty(c, hw, dtype=torch.float16, device=DEV)
    scale = 1 / math.sqrt(c)
    rows_max, blocks = attn_row_blocks(hw) if hw > ATTN_LONG_FROM else (hw, [(0, hw)])
    scores = torch.empty((rows_max, hw), dtype=torch.float32, device=DEV)
    probs = scores.view(torch.float16)
    softmax = ops.softmax_rows_long_f32 if hw > ATTN_LONG_FROM else ops.softmax_rows_f32

    def fused():
        ops.attn_wide(q, k, v, o_f, ldq=c, ldk=c, ldv=c, ldo=c, batch=1, seq=hw, head_dim=c, scale=scale)

    def composed():
        ops.gemm(wv, x, vt, m=c, n=hw, cin=c)
        for r0, r1 in blocks:
            ops.gemm_f32out(q[r0:r1], k, scores, m=r1 - r0, n=hw, k=c)
            softmax(scores, probs, rows=r1 - r0, cols=hw, scale=scale, ld=hw, ldo=2 * hw)
            ops.gemm(probs[:r1 - r0, :hw], vt, o_c[r0:r1], m=r1 - r0, n=c, cin=hw, lda=2 * hw, bias=bv)

    tf, tc = [], []
    for _ in range(3):                                   # arms alternate
        tf += timed(fused, reps)
        tc += timed(composed, reps)
    diff = float((o_f.float() - o_c.float()).norm() / o_c.float().norm())
    fl = 4.0 * hw * hw * c
    for name, t in (("fused", tf), ("composed core", tc)):
        med = statistics.median(t)
        lines.append(f"  {hw:6d} tokens x {c}: {name:14s} median {med:8.3f} ms (min {min(t):.3f}, max {max(t):.3f}, n={len(t)})  "
                     f"{fl / med / 1e9:7.1f} TFLOP/s")
    lines.append(f"  {hw:6d} tokens: composed / fused = {statistics.median(tc) / statistics.median(tf):.2f}x, outputs differ by rel-L2 {diff:.1e}")


def decode(h, w, frames, lines):
    cfg = VAEDecoderConfig.svd()
    sd = random_state_dict(cfg, seed=3)
    z = (torch.randn(frames, 4, h // 8, w // 8, generator=torch.Generator().manual_seed(31)) * 4.0).half().to(DEV)
    outs = {}
    for route in ("composed", "fused"):
        dec = TemporalDecoderHIP(cfg, sd, DEV, attention=route)
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        t = timed(lambda: dec.decode(z, frames), 3)
        outs[route] = dec.decode(z, frames).float()
        lines.append(f"  decode {h} x {w} x {frames} frames, {route:8s}: median {statistics.median(t):9.1f} ms (min {min(t):.1f}, max "
                     f"{max(t):.1f}), peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:9.0f} MiB")
        del dec
    lines.append(f"  decode {h} x {w}: routes differ by rel-L2 {float((outs['fused'] - outs['composed']).norm() / outs['composed'].norm()):.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_wide_timing.txt"))
    a = ap.parse_args()
    lines = [f"tools/attn_wide_timing.py on {torch.cuda.get_device_name(0)}: events around single calls, arms alternating in one "
             f"process, random weights", "attention core, one image, width 512 (FLOP = 4 seq^2 d):"]
    for hw in (9216, 20736):
        core(hw, 512, a.reps, lines)
    lines.append("whole decode (TemporalDecoderHIP, SVD widths):")
    for h, w in ((576, 1024), (864, 1536)):
        decode(h, w, a.frames, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
