#!/usr/bin/env python3
"""What a lossless animated WebP costs, per video of 14 frames of 576 x 1024 on the device (profiles/webp_timing.txt):

  * the GPU route over a grid of pred_bits x group_bits: sp_webp_transform_u8, sp_webp_code, the device-to-host copy of the
    lengths and the used bytes plus the RIFF wrapping (collect_streams + write_webp; the wrapping alone is timed as well: the
    container has no checksum), and WebpEncoder.encode_animation as a whole (host clock around a call that ends synchronised);
  * two baselines on the same box in the same run: the device-to-host copy of the uint8 frames plus Pillow's lossless WebP
    writer on the host (save_all, default settings, one thread; timed in PILLOW_ROUNDS rounds only, it takes seconds), and
    PngEncoder.encode_apng (filter, deflate, copy, and the host's CRC-32 over every chunk);
  * the bytes of the files of all of them.

Input: a smooth two-sinusoid colour field that moves from frame to frame plus sigma = 8 noise (the field of png_timing.py:
its channels carry independent noise, so subtract green does not pay there), and the same field's green with red and blue
following it at +20 / -15 and noise of +-2 (channels that move together, as a real picture's do).
Device events around the device work, a host clock around what ends on the host; NWARM warm-up rounds, then the median,
minimum and maximum of NREP rounds, the routes alternating round by round.
usage: webp_timing.py   (environment: NREP=5 NWARM=1 PILLOW_ROUNDS=1)"""
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
from vdpp_amd.models.image_io import WEBP_GROUP_BITS, WEBP_PRED_BITS, PngEncoder, WebpEncoder, write_webp

NREP, NWARM = int(os.environ.get("NREP", 5)), int(os.environ.get("NWARM", 1))
PILLOW_ROUNDS = int(os.environ.get("PILLOW_ROUNDS", 1))
F, H, W = 14, 576, 1024
PRED_BITS, GROUP_BITS = (2, 3, 4, 5), (3, 4, 5)
FPS = 7
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


def correlated(frames, seed=1):
    rng = np.random.default_rng(seed)
    g = frames[..., 1].astype(np.int32)
    r = np.clip(g + 20 + rng.integers(-2, 3, g.shape), 0, 255)
    b = np.clip(g - 15 + rng.integers(-2, 3, g.shape), 0, 255)
    return np.stack([r, g, b], -1).astype(np.uint8)


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
    ims[0].save(buf, format="WEBP", save_all=True, append_images=ims[1:], lossless=True, loop=0, duration=round(1000 / FPS))
    return buf.getvalue()


def med(t):
    return sorted(t)[len(t) // 2]


def line(name, t):
    return f"  {name}: median {med(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f}; {len(t)} rounds)"


def decoded(data):
    with Image.open(io.BytesIO(data)) as im:
        out = []
        for k in range(im.n_frames):
            im.seek(k)
            out.append(np.asarray(im.convert("RGB")))
        return out


def measure(name, host_frames):
    frames = torch.from_numpy(host_frames).to(dev)
    grid = [(p, g) for p in PRED_BITS for g in GROUP_BITS]
    encs = {pg: WebpEncoder(dev, H, W, pred_bits=pg[0], group_bits=pg[1]) for pg in grid}
    png = PngEncoder(dev, H, W, assemble="host")              # the route the lines name (the device route: profiles/png_timing.txt)
    keys = [f"{k}{pg}" for pg in grid for k in ("transform", "code", "collect", "wrap", "encode")] + ["apng", "raw_copy", "pillow"]
    t = {k: [] for k in keys}
    sizes, ours = {}, {}
    for it in range(NWARM + NREP):
        r_ = {}
        for pg, enc in encs.items():
            n, bs = frames.shape[0], 1 << pg[0]
            residual = enc._buf("residual", (n, H, W, 4), torch.uint8)
            modes = enc._buf("modes", (n, -(-H // bs), -(-W // bs)), torch.uint8)
            flags = enc._buf("flags", (n,), torch.int32)
            out, lens = enc._buf("stream", (n, enc.cap), torch.uint8), enc._buf("len", (n,), torch.int32)
            ws = enc._buf("ws", (ops.webp_ws_bytes(n, H, W, *pg),), torch.uint8)
            r_[f"transform{pg}"], _ = device_ms(lambda: ops.webp_transform(frames, residual, modes, flags, ws, pred_bits=pg[0]))
            r_[f"code{pg}"], _ = device_ms(lambda: ops.webp_code(residual, modes, flags, out, lens, ws, pred_bits=pg[0], group_bits=pg[1]))
            r_[f"collect{pg}"], data = host_ms(lambda: write_webp(None, enc.collect_streams(out, lens), W, H, FPS))
            streams = enc.collect_streams(out, lens)
            r_[f"wrap{pg}"], _ = host_ms(lambda: write_webp(None, streams, W, H, FPS))
            r_[f"encode{pg}"], again = host_ms(lambda: enc.encode_animation(frames, FPS))
            assert data == again
            sizes[pg], ours[pg] = len(data), data
        r_["apng"], apng = host_ms(lambda: png.encode_apng(frames, FPS))
        sizes["apng"] = len(apng)
        r_["raw_copy"], raw = host_ms(lambda: frames.cpu().numpy())
        if it >= NWARM + NREP - PILLOW_ROUNDS:
            r_["pillow"], theirs = host_ms(lambda: pillow(raw))
            sizes["pillow"] = len(theirs)
        if it >= NWARM:
            for k in keys:
                if k in r_:
                    t[k].append(r_[k])
    for pg in ((WEBP_PRED_BITS, WEBP_GROUP_BITS), grid[0], grid[-1]):     # the files open in libwebp and give the frames back
        assert all(np.array_equal(a, b) for a, b in zip(decoded(ours[pg]), host_frames)), pg

    print(f"---- input: {name}")
    host = med(t["raw_copy"]) + med(t["pillow"])
    for pg in grid:
        e = med(t[f"encode{pg}"])
        print(f"GPU route, pred_bits {pg[0]} (blocks of {1 << pg[0]}), group_bits {pg[1]} ({F * -(-H // (1 << pg[1]))} strips of {1 << pg[1]} rows):")
        print(line("sp_webp_transform_u8, two kernels and a memset (device events)", t[f"transform{pg}"]))
        print(line("sp_webp_code, four kernels (device events)", t[f"code{pg}"]))
        print(line("lengths, then the used bytes to the host, the RIFF chunks put together (host clock)", t[f"collect{pg}"]))
        print(line("  of which the RIFF wrapping alone (host clock)", t[f"wrap{pg}"]))
        print(line("WebpEncoder.encode_animation, all of the above in one call (host clock)", t[f"encode{pg}"]))
        print(f"  file {sizes[pg]} bytes, {100.0 * (sizes[pg] / sizes['apng'] - 1):+.2f} % against the APNG, "
              f"{100.0 * (sizes[pg] / sizes['pillow'] - 1):+.2f} % against Pillow's WebP; PngEncoder.encode_apng over this call, "
              f"medians: {med(t['apng']) / e:.2f} x; host route over this call: {host / e:.0f} x; {e / 1e3:.4f} s of the {VIDEO_S} s a video takes")
    print("baselines:")
    print(line("PngEncoder.encode_apng, strips of 16 rows: kernels, copy, chunks and the host's CRC-32 (host clock)", t["apng"]))
    print(f"  file {sizes['apng']} bytes")
    print(line(f"the uint8 frames to the host, {frames.numel() / 1e6:.1f} MB (host clock)", t["raw_copy"]))
    print(line("Pillow's WebP writer on the frames, lossless=True, save_all, default settings, 1 thread (host clock)", t["pillow"]))
    print(f"  file {sizes['pillow']} bytes")
    fastest = min(grid, key=lambda pg: med(t[f"encode{pg}"]))
    smallest = min(grid, key=lambda pg: sizes[pg])
    print(f"fastest whole call: pred_bits, group_bits = {fastest}; smallest file: {smallest}; the defaults are "
          f"{(WEBP_PRED_BITS, WEBP_GROUP_BITS)}")


def main():
    print(f"device: {torch.cuda.get_device_name(0)}; {F} frames of {H}x{W} at {FPS} fps; {NWARM} warm-up rounds, then {NREP} timed rounds "
          f"per line (Pillow's writer: the last {PILLOW_ROUNDS})")
    base = scene()
    measure("independent noise per channel (the field of png_timing.py)", base)
    measure("channels that follow green", correlated(base))


with torch.no_grad():
    main()
