#!/usr/bin/env python3
"""What an animated GIF costs, per video of 14 frames of 576 x 1024 on the device (profiles/gif_timing.txt):

  * the GPU route at strip_rows 8, 16 and 32: sp_gif_quantise_u8, sp_gif_lzw, the device-to-host copy of the palettes, the
    lengths and the used bytes plus the assembly of the file (GifEncoder.collect), and GifEncoder.encode as a whole (host clock
    around a call that ends synchronised);
  * the route without the kernels: the device-to-host copy of the uint8 frames, then Pillow's GIF writer on the host (what
    save_frames did with a device tensor before; one thread);
  * the bytes of the files of both, and of one dictionary per frame (strip_rows = 576) for the cost of the strips.

Input: a smooth two-sinusoid colour field that moves from frame to frame plus sigma = 8 noise (the field of the tests).
Device events around the device work, a host clock around what ends on the host; NWARM warm-up rounds, then the median,
minimum and maximum of NREP rounds, the routes alternating round by round.
usage: gif_timing.py   (environment: NREP=5 NWARM=1 FPS=7)"""
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

import vdpp_amd  # noqa
from vdpp_amd.hip import ops
from vdpp_amd.models.image_io import GifEncoder

NREP, NWARM = int(os.environ.get("NREP", 5)), int(os.environ.get("NWARM", 1))
FPS = int(os.environ.get("FPS", 7))
F, H, W = 14, 576, 1024
STRIP_ROWS = (8, 16, 32)
VIDEO_S = 1.16                       # one MI355X generates such a video in 1.16 s (README: 0.86 videos/s)
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


def pillow(frames):
    ims = [Image.fromarray(f) for f in frames]
    buf = io.BytesIO()
    ims[0].save(buf, format="GIF", save_all=True, append_images=ims[1:], loop=0, duration=1000.0 / FPS)
    return buf.getvalue()


def med(t):
    return sorted(t)[len(t) // 2]


def line(name, t):
    return f"  {name}: median {med(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f})"


def main():
    frames = torch.from_numpy(scene()).to(dev)
    encs = {r: GifEncoder(dev, H, W, strip_rows=r, fps=FPS) for r in STRIP_ROWS}
    keys = [f"{k}{r}" for r in STRIP_ROWS for k in ("quantise", "lzw", "collect", "encode")] + ["raw_copy", "pillow"]
    t = {k: [] for k in keys}
    sizes = {}
    for it in range(NWARM + NREP):
        r_ = {}
        for r, enc in encs.items():
            n = frames.shape[0]
            pal, idx = enc._buf("palette", (n, 256, 3), torch.uint8), enc._buf("index", (n, H, W), torch.uint8)
            out, lens = enc._buf("stream", (n, enc.cap), torch.uint8), enc._buf("len", (n,), torch.int32)
            ws = enc._buf("ws", (ops.gif_ws_bytes(n, H, W, r),), torch.uint8)
            r_[f"quantise{r}"], _ = device_ms(lambda: ops.gif_quantise(frames, pal, idx, ws))
            r_[f"lzw{r}"], _ = device_ms(lambda: ops.gif_lzw(idx, out, lens, ws, strip_rows=r))
            r_[f"collect{r}"], ours = host_ms(lambda: enc.collect(pal, out, lens))
            r_[f"encode{r}"], again = host_ms(lambda: enc.encode(frames))
            assert ours == again
            sizes[r] = len(ours)
        r_["raw_copy"], raw = host_ms(lambda: frames.cpu().numpy())
        r_["pillow"], theirs = host_ms(lambda: pillow(raw))
        sizes["pillow"] = len(theirs)
        if it >= NWARM:
            for k in keys:
                t[k].append(r_[k])
    sizes["one"] = len(GifEncoder(dev, H, W, strip_rows=H, fps=FPS).encode(frames))
    with Image.open(io.BytesIO(ours)) as im:                # the last file still opens
        assert im.n_frames == F and im.size == (W, H)

    print(f"device: {torch.cuda.get_device_name(0)}; {F} frames of {H}x{W}; {NWARM} warm-up rounds, then {NREP} timed rounds per line")
    host = med(t["raw_copy"]) + med(t["pillow"])
    for r in STRIP_ROWS:
        print(f"GPU route, strip_rows {r} ({F * -(-H // r)} strips):")
        print(line("sp_gif_quantise_u8, five kernels (device events)", t[f"quantise{r}"]))
        print(line("sp_gif_lzw, three kernels (device events)", t[f"lzw{r}"]))
        print(line("palettes, lengths, then the used bytes to the host, file put together (host clock)", t[f"collect{r}"]))
        print(line("GifEncoder.encode, all of the above in one call (host clock)", t[f"encode{r}"]))
        e = med(t[f"encode{r}"])
        print(f"  file {sizes[r]} bytes, {100.0 * (sizes[r] / sizes['one'] - 1):+.2f} % over one dictionary per frame ({sizes['one']} bytes); "
              f"host route over this route, medians: {host / e:.1f} x; {e / 1e3:.3f} s of the {VIDEO_S} s a video takes")
    print("host route:")
    print(line(f"the uint8 frames to the host, {frames.numel() / 1e6:.1f} MB (host clock)", t["raw_copy"]))
    print(line("Pillow's GIF writer on the frames, 1 thread (host clock)", t["pillow"]))
    print(f"  file {sizes['pillow']} bytes")
    best = min(STRIP_ROWS, key=lambda r: med(t[f"encode{r}"]))
    ok = all(med(t[f"encode{r}"]) < min(host, VIDEO_S * 1e3) for r in STRIP_ROWS)
    print(f"fastest strip_rows: {best}; every GPU route below the host route and below {VIDEO_S} s: {ok}")


with torch.no_grad():
    main()
