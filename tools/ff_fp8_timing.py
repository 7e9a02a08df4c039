#!/usr/bin/env python3
"""FF1 of the GEGLU feed-forwards, fp16 against fp8, kernel level: at each shape of a two-video forward the fp16
contraction with its folded LayerNorm (``ops.gemm(..., ln_stats=, geglu=True)``) against LayerNorm + e4m3 quantisation
(``ops.ln_quant_f8``) followed by the W8A8 contraction (``ops.gemm_f8``).  Both arms read the same rows and the same row
statistics (the statistics pass is common to both and not timed) and alternate in one process: ROUNDS rounds of ITERS
calls each between two events, median and best per arm.  usage: ff_fp8_timing.py [--rounds 7] [--iters 20]"""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd.hip import ops
from vdpp_amd.models import weights as W

dev = torch.device("cuda:0")
SHAPES = [("level 0 spatial ff", 2 * 14 * 9216, 320), ("level 1 spatial ff", 2 * 14 * 2304, 640),
          ("level 2 spatial ff", 2 * 14 * 576, 1280), ("level 0 temporal ff_in", 2 * 14 * 9216, 320)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.iters          # us per call


print(f"{torch.cuda.get_device_name(0)}; us per call, median (best) of {args.rounds} rounds x {args.iters} calls, arms alternating")
for name, m, c in SHAPES:
    n = 8 * c
    g = torch.Generator().manual_seed(c)
    x = torch.randn(m, c, generator=g).half().to(dev)
    w = torch.randn(n, c, generator=g) / c ** 0.5
    wi, bi = W.interleave_geglu(w, torch.randn(n, generator=g))
    wi, bi = wi.to(dev), bi.to(dev)
    colsum = wi.float().sum(1).contiguous()
    w8, sw = (t.to(dev) for t in W.pack_linear_f8(wi.float()))
    st = torch.empty(m, 2, device=dev)
    ops.ln_stats(x, st, rows=m, c=c)
    q, sa = torch.empty(m, c, dtype=torch.uint8, device=dev), torch.empty(m, device=dev)
    out16, out8 = (torch.empty(m, n // 2, dtype=torch.float16, device=dev) for _ in range(2))
    arms = {
        "fp16 ff1 (folded LayerNorm)": lambda: ops.gemm(x, wi, out16, m=m, n=n, cin=c, bias=bi, geglu=True, ln_stats=st, ln_colsum=colsum),
        "ln_quant_f8": lambda: ops.ln_quant_f8(x, st, q, sa, rows=m, c=c),
        "gemm_f8": lambda: ops.gemm_f8(q, sa, w8, sw, bi, out8, m=m, n=n, k=c, geglu=True),
        "ln_quant_f8 + gemm_f8": lambda: (ops.ln_quant_f8(x, st, q, sa, rows=m, c=c),
                                          ops.gemm_f8(q, sa, w8, sw, bi, out8, m=m, n=n, k=c, geglu=True)),
    }
    for fn in arms.values():
        fn(); fn()
    torch.cuda.synchronize()
    kern16 = ops.load().sp_gemm_last_kernel().decode()
    rel = float((out8.float() - out16.float()).norm() / out16.float().norm())
    t = {a: [] for a in arms}
    for _ in range(args.rounds):
        for a, fn in arms.items():
            t[a].append(timed(fn))
    print(f"--- {name}: m = {m}, K = {c}, N = {n} ({2.0 * m * n * c / 1e12:.2f} TFLOP, {m * n / 1e6:.0f} MB hidden written); "
          f"fp8 vs fp16 output rel-L2 {rel:.2e}")
    base = statistics.median(t["fp16 ff1 (folded LayerNorm)"])
    for a in arms:
        med = statistics.median(t[a])
        print(f"  {a:30s} {med:9.1f} ({min(t[a]):9.1f}) us   x{base / med:5.2f} vs fp16   {2.0 * m * n * c / med / 1e6:7.1f} TFLOP/s"
              if "gemm" in a or "ff1" in a else f"  {a:30s} {med:9.1f} ({min(t[a]):9.1f}) us", flush=True)
