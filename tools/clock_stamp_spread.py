#!/usr/bin/env python3
"""What `ops.ClockStamps.ghz()` rests on: do the CUs of one XCD share a shader-clock counter (s_memtime), and do two launches of
`sp_clock_stamp` land on the same CUs?  Two stamps around 200 contractions (8192 x 5120 x 1280, about 20 ms: the stretch of
tests/test_kernels_gpu.py::test_clock_stamps_bracket_work), TRIES times, each time twice:

  64 workgroups    a stamp of 64 one-wave workgroups, the first workgroup of each XCD in the first stamp paired with the first of
                   that XCD in the last one, the mean over the XCDs (how the stamps were paired before CUs were noted)
  1,024, by CU     ops.ClockStamps as it is: 1,024 workgroups, paired CU by CU, each XCD's median, the mean over the XCDs

and per XCD how far apart the counters of its CUs are within ONE stamp, and how far apart the CU-by-CU ratios are.
usage: clock_stamp_spread.py [--tries 3] [--commit TEXT] [--out profiles/clock_stamp_per_cu.txt]"""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--tries", type=int, default=3)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clock_stamp_per_cu.txt"))
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd.hip import ops

M, N, K, CALLS = 8192, 5120, 1280, 200


def bracket(blocks):
    """Two stamps of ``blocks`` workgroups around the stretch: the two [blocks][4] records (place, shader, 100 MHz, 1)."""
    buf = torch.zeros((2, blocks, 4), dtype=torch.int64, device=dev)
    lib, stream = ops.load(), torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    assert lib.sp_clock_stamp(buf[0].data_ptr(), blocks, stream) == 0
    for _ in range(CALLS):
        ops.gemm(a, w, out, m=M, n=N, cin=K)
    assert lib.sp_clock_stamp(buf[1].data_ptr(), blocks, stream) == 0
    torch.cuda.synchronize()
    return buf.cpu()


def ratio(f, l):
    return 0.1 * (l[1] - f[1]) / (l[2] - f[2])


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    a = torch.randn(M, K, device=dev, dtype=torch.float16)
    w = torch.randn(N, K, device=dev, dtype=torch.float16) * 0.02
    out = torch.empty(M, N, device=dev, dtype=torch.float16)
    for _ in range(3):
        ops.gemm(a, w, out, m=M, n=N, cin=K)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lines = [f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs; commit: "
             f"{commit or 'unknown'}; two sp_clock_stamp launches around {CALLS} contractions of {M} x {N} x {K} (fp16), {args.tries} tries",
             "place of a workgroup = XCD (HW_REG_XCC_ID) and CU within it (HW_REG_HW_ID: shader engine, array, CU); ratio = 0.1 GHz x "
             "shader ticks / 100 MHz ticks between the two stamps"]
    for t in range(args.tries):
        small = bracket(64)
        per_xcd, same = [], 0
        for x in sorted(set((small[0][:, 0] & 15).tolist()) & set((small[1][:, 0] & 15).tolist())):
            f = small[0][(small[0][:, 0] & 15) == x][0].tolist()
            l = small[1][(small[1][:, 0] & 15) == x][0].tolist()
            per_xcd.append(ratio(f, l))
            same += f[0] == l[0]
        shared = len(set(small[0][:, 0].tolist()) & set(small[1][:, 0].tolist()))
        lines.append(f"try {t}: 64 workgroups, first of each XCD paired: {sum(per_xcd) / len(per_xcd):8.3f} GHz   per XCD: "
                     f"{' '.join(f'{r:.2f}' for r in per_xcd)}   ({same} of {len(per_xcd)} pairs on one CU; the two stamps share "
                     f"{shared} of their CUs)")
        st = ops.ClockStamps(dev, 2)
        torch.cuda.synchronize()
        st.stamp()
        for _ in range(CALLS):
            ops.gemm(a, w, out, m=M, n=N, cin=K)
        st.stamp()
        torch.cuda.synchronize()
        ghz, secs, xcds = st.ghz()
        b = st.buf[:2].cpu()
        rows = [{r[0]: r for r in reversed(s.tolist())} for s in (b[0], b[1])]
        both = sorted(rows[0].keys() & rows[1].keys())
        lines.append(f"try {t}: {st.BLOCKS} workgroups, paired CU by CU:         {ghz:8.3f} GHz over {secs * 1e3:.2f} ms, {xcds} XCDs; CUs in the "
                     f"first stamp {len(rows[0])}, in the last {len(rows[1])}, in both {len(both)}")
        for x in sorted({p & 15 for p in both}):
            rs = sorted(ratio(rows[0][p], rows[1][p]) for p in both if p & 15 == x)
            ticks = [rows[0][p][1] for p in rows[0] if p & 15 == x]
            lines.append(f"    XCD {x}: {len(rs):3d} CUs, their counters within the first stamp {max(ticks) - min(ticks):>12,d} ticks apart; "
                         f"CU-by-CU ratio min {rs[0]:.4f} median {rs[len(rs) // 2]:.4f} max {rs[-1]:.4f}")
    # what a stamp costs the stream it is taken on (bench.py --full takes one behind every finished video)
    buf = torch.zeros((1024, 4), dtype=torch.int64, device=dev)
    lib, stream = ops.load(), torch.cuda.current_stream().cuda_stream
    for blocks in (64, 1024):
        us = []
        for r in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                lib.sp_clock_stamp(buf.data_ptr(), blocks, stream)
            e1.record(); e1.synchronize()
            us.append(e0.elapsed_time(e1) * 10.0)
        lines.append(f"one stamp of {blocks:4d} workgroups, device events around 100 back-to-back launches, 5 rounds: median "
                     f"{sorted(us)[2]:.2f} us  min {min(us):.2f}  max {max(us):.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
