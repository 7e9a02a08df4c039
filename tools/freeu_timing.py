#!/usr/bin/env python3
"""FreeU (sp_freeu_f16, csrc/freeu.hip) alone at the ten sites of a two-video SVD forward (28 images: 1,280 running channels
at 9 x 16 three times, 18 x 32 three times and 36 x 64 once; 640 at 36 x 64 twice and 72 x 128 once), versions 1 and 2, with
the bytes the three passes move and the rate that makes, beside a GroupNorm of the same buffer (sp_groupnorm_ld_f16: its
statistics pass and gn_apply_kernel, three passes over the buffer) as a bandwidth yardstick: events around single calls on
a buffer refilled before each one (the call works in place).  Then whole forwards through tools/ab_forward.py in a child
process.  Writes profiles/freeu_timing.txt.   usage: freeu_timing.py [--reps 7] [--no-forwards]"""
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
from vdpp_amd.models.unet_spec import UNetConfig, up_block_plan

DEV = "cuda:0"
FREEU = (1.3, 1.4, 0.9, 0.2)          # b1, b2, s1, s2


def sites(cfg, h, w):
    """(c_left, c_right, h, w, b, s) in the order the up path meets them."""
    c0, layers = cfg.block_out_channels[0], cfg.layers_per_block + 1
    pairs = {4 * c0: (FREEU[0], FREEU[2]), 2 * c0: (FREEU[1], FREEU[3])}
    shift = len(cfg.block_out_channels) - 1
    sh, sw = h >> shift, w >> shift
    for in_ch, out_ch, prev, _attn, _heads, ups in up_block_plan(cfg):
        for j in range(layers):
            rin, skip = prev if j == 0 else out_ch, in_ch if j == layers - 1 else out_ch
            if rin in pairs:
                yield (rin, skip, sh, sw) + pairs[rin]
        if ups:
            sh, sw = 2 * sh, 2 * sw


def timed(fn, refill, reps):
    """Milliseconds of `reps` single calls (events around each, the buffer refilled in front), after two warm-up calls."""
    out = []
    for i in range(reps + 2):
        refill()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        if i >= 2:
            out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--images", type=int, default=28)
    ap.add_argument("--no-forwards", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeu_timing.txt"))
    a = ap.parse_args()
    cfg, n = UNetConfig.svd(), a.images
    lines = [f"tools/freeu_timing.py on {torch.cuda.get_device_name(0)}: events around single calls, {n} images, Gaussian data, "
             f"freeu = {FREEU}; bytes: version 2 reads c_left (means), reads c_right (coefficients), reads and writes c_right and "
             f"c_left/2 (apply); version 1 has no mean pass; GroupNorm: x read twice, y written once.  Every call follows a refill of its "
             f"buffer: what the last-level cache keeps of it is served from there, so the small sites show a cache rate, not HBM's."]
    total = {1: 0.0, 2: 0.0}
    for cl, cr, h, w, b, s in sites(cfg, 72, 128):
        rows, c = n * h * w, cl + cr
        src = torch.randn(rows, c, generator=torch.Generator().manual_seed(h + c)).half().to(DEV)
        cat, y = torch.empty_like(src), torch.empty_like(src)
        ws = torch.empty(ops.freeu_ws_bytes(n, h, w, cl, cr), dtype=torch.uint8, device=DEV)
        gws = torch.empty(ops.groupnorm_ws_bytes(n, h * w, c, 32), dtype=torch.uint8, device=DEV)
        g32, b32 = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
        lines.append(f"c_left {cl}, c_right {cr}, {h} x {w}  ({rows * c * 2 / 1e6:.1f} MB buffer)")
        for version in (1, 2):
            t = timed(lambda: ops.freeu(cat, ws, n_img=n, h=h, w=w, c_left=cl, c_right=cr, b=b, s=s, version=version),
                      lambda: cat.copy_(src), a.reps)
            nbytes = 2.0 * rows * ((cl if version == 2 else 0) + cl + 3 * cr)
            med = statistics.median(t)
            total[version] += med
            lines.append(f"  sp_freeu_f16 version {version}       median {med * 1e3:8.1f} us (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}, n={len(t)})"
                         f"  {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e9:6.2f} TB/s")
        t = timed(lambda: ops.groupnorm(cat, g32, b32, y, instances=n, rows=h * w, c=c, groups=32, eps=1e-6, silu=True, ws=gws),
                  lambda: cat.copy_(src), a.reps)
        med, nbytes = statistics.median(t), 6.0 * rows * c
        lines.append(f"  GroupNorm + SiLU of the buffer  median {med * 1e3:8.1f} us (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}, n={len(t)})"
                     f"  {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e9:6.2f} TB/s")
    lines.append(f"sum of the medians over the ten sites: version 1 {total[1]:.3f} ms, version 2 {total[2]:.3f} ms per two-video forward")
    if not a.no_forwards:
        torch.cuda.synchronize()
        arm = "unet:freeu=" + "/".join(map(str, FREEU))
        lines.append(f"whole forwards (tools/ab_forward.py --rounds 3 --steps 4 base {arm} {arm},unet:freeu_version=1; a child process; "
                     f"with FreeU on, the ten up resnets' first norms take their statistics pass again):")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_forward.py"), "--rounds", "3", "--steps", "4", "base", arm,
                              arm + ",unet:freeu_version=1"], capture_output=True, text=True, check=True).stdout
        lines += ["  " + ln for ln in out.splitlines() if "ms per video" in ln]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
