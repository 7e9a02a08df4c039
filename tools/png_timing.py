#!/usr/bin/env python3
"""What lossless PNG frames cost, per video of 14 frames of 576 x 1024 on the device (profiles/png_timing.txt):

  * the GPU route at strip_rows 4, 8, 16 and 32: sp_png_filter_u8, sp_png_deflate, the device-to-host copy of the lengths and
    the used bytes plus the chunks and their CRC-32 (PngEncoder.collect; the CRC alone is timed as well), and
    PngEncoder.encode as a whole (host clock around a call that ends synchronised);
  * the route without the kernels: the device-to-host copy of the uint8 frames, then Pillow's PNG writer per frame on the host
    (what save_frames did with a device tensor before; one thread);
  * the bytes of the files of both, and of one strip per frame (strip_rows = 576) for the cost of the strips;
  * at the default strip height, the two ways to the files in the same run: assemble="host" (the streams to the host,
    png_file / write_apng and zlib.crc32 there) and assemble="device" (sp_png_wrap: chunks, CRC-32 and an animation's layout on
    the device, finished files to the host), PngEncoder.encode and encode_apng under each, and device events around
    sp_crc32_rows over the streams and around sp_png_wrap (stills, animation) alone.  Both routes must give the same bytes.

The strip heights are compared on the host route, whose parts the lines name.

The default strip height is the fastest of the four whose files are within 1 % of one strip per frame.
Input: a smooth two-sinusoid colour field that moves from frame to frame plus sigma = 8 noise (the field of the tests).
Device events around the device work, a host clock around what ends on the host; NWARM warm-up rounds, then the median,
minimum and maximum of NREP rounds, the routes alternating round by round.
usage: png_timing.py   (environment: NREP=5 NWARM=1)"""
import io
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

import vdpp_amd  # noqa
from vdpp_amd.hip import ops
from vdpp_amd.models.image_io import PngEncoder

NREP, NWARM = int(os.environ.get("NREP", 5)), int(os.environ.get("NWARM", 1))
F, H, W = 14, 576, 1024
STRIP_ROWS = (4, 8, 16, 32)
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
    files = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="PNG")
        files.append(buf.getvalue())
    return files


def med(t):
    return sorted(t)[len(t) // 2]


def line(name, t):
    return f"  {name}: median {med(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f})"


def main():
    host_frames = scene()
    frames = torch.from_numpy(host_frames).to(dev)
    encs = {r: PngEncoder(dev, H, W, strip_rows=r, assemble="host") for r in STRIP_ROWS}
    routes = {a: PngEncoder(dev, H, W, assemble=a) for a in ("host", "device")}
    keys = [f"{k}{r}" for r in STRIP_ROWS for k in ("filter", "deflate", "collect", "crc", "encode")] + ["raw_copy", "pillow"]
    keys += [f"{k}_{a}" for a in routes for k in ("encode", "apng")] + ["crc_rows", "wrap_stills", "wrap_apng"]
    t = {k: [] for k in keys}
    sizes = {}
    for it in range(NWARM + NREP):
        r_ = {}
        for r, enc in encs.items():
            n = frames.shape[0]
            flt = enc._buf("filtered", (n, H, 1 + 3 * W), torch.uint8)
            out, lens = enc._buf("stream", (n, enc.cap), torch.uint8), enc._buf("len", (n,), torch.int32)
            ws = enc._buf("ws", (ops.png_ws_bytes(n, H, W, r),), torch.uint8)
            r_[f"filter{r}"], _ = device_ms(lambda: ops.png_filter(frames, flt))
            r_[f"deflate{r}"], _ = device_ms(lambda: ops.png_deflate(flt, out, lens, ws, strip_rows=r))
            r_[f"collect{r}"], ours = host_ms(lambda: enc.collect(out, lens))
            streams = enc.collect_streams(out, lens)
            r_[f"crc{r}"], _ = host_ms(lambda: [zlib.crc32(s, zlib.crc32(b"IDAT")) for s in streams])
            r_[f"encode{r}"], again = host_ms(lambda: enc.encode(frames))
            assert ours == again
            sizes[r] = sum(len(f) for f in ours)
        made = {}
        for a, enc in routes.items():
            r_[f"encode_{a}"], stills = host_ms(lambda: enc.encode(frames))
            r_[f"apng_{a}"], movie = host_ms(lambda: enc.encode_apng(frames, 7))
            made[a] = (stills, movie)
        assert made["host"] == made["device"], "the two routes give different bytes"
        enc, n = routes["device"], frames.shape[0]
        out, lens = enc.enqueue(frames)
        crc = enc._buf("crc", (n,), torch.int32)
        crc_ws = enc._buf("crc_ws", (ops.crc32_ws_bytes(n, enc.cap),), torch.uint8)
        files, file_lens = enc._buf("files", (n, ops.png_file_bytes(H, W, enc.strip_rows)), torch.uint8), enc._buf("file_len", (n,), torch.int32)
        movie_buf = enc._buf("apng", (ops.apng_file_bytes(n, H, W, enc.strip_rows),), torch.uint8)
        wrap_ws = enc._buf("wrap_ws", (ops.png_wrap_ws_bytes(n, enc.cap),), torch.uint8)
        r_["crc_rows"], _ = device_ms(lambda: ops.crc32_rows(out, lens, crc, crc_ws))
        r_["wrap_stills"], _ = device_ms(lambda: ops.png_wrap(out, lens, files, file_lens, wrap_ws, height=H, width=W))
        r_["wrap_apng"], _ = device_ms(lambda: ops.png_wrap(out, lens, movie_buf, file_lens, wrap_ws, height=H, width=W, animate=True))
        r_["raw_copy"], raw = host_ms(lambda: frames.cpu().numpy())
        r_["pillow"], theirs = host_ms(lambda: pillow(raw))
        sizes["pillow"] = sum(len(f) for f in theirs)
        if it >= NWARM:
            for k in keys:
                t[k].append(r_[k])
    sizes["one"] = sum(len(f) for f in PngEncoder(dev, H, W, strip_rows=H).encode(frames))
    for k, data in enumerate(ours):                          # the last files still open, and give the frames back
        with Image.open(io.BytesIO(data)) as im:
            assert im.size == (W, H) and np.array_equal(np.asarray(im), host_frames[k])

    print(f"device: {torch.cuda.get_device_name(0)}; {F} frames of {H}x{W}; {NWARM} warm-up rounds, then {NREP} timed rounds per line")
    host = med(t["raw_copy"]) + med(t["pillow"])
    for r in STRIP_ROWS:
        print(f"GPU route, files put together on the host, strip_rows {r} ({F * -(-H // r)} strips):")
        print(line("sp_png_filter_u8, one kernel (device events)", t[f"filter{r}"]))
        print(line("sp_png_deflate, three kernels (device events)", t[f"deflate{r}"]))
        print(line("lengths, then the used bytes to the host, chunks and CRC-32, files put together (host clock)", t[f"collect{r}"]))
        print(line("  of which zlib.crc32 over the IDAT payloads (host clock)", t[f"crc{r}"]))
        print(line("PngEncoder.encode, all of the above in one call (host clock)", t[f"encode{r}"]))
        e = med(t[f"encode{r}"])
        print(f"  files {sizes[r]} bytes, {100.0 * (sizes[r] / sizes['one'] - 1):+.2f} % over one strip per frame ({sizes['one']} bytes), "
              f"{100.0 * (sizes[r] / sizes['pillow'] - 1):+.2f} % against Pillow; host route over this route, medians: {host / e:.1f} x; "
              f"{e / 1e3:.3f} s of the {VIDEO_S} s a video takes")
    print("host route:")
    print(line(f"the uint8 frames to the host, {frames.numel() / 1e6:.1f} MB (host clock)", t["raw_copy"]))
    print(line("Pillow's PNG writer on the frames, default settings, 1 thread (host clock)", t["pillow"]))
    print(f"  files {sizes['pillow']} bytes")
    print(f"files put together on the host and on the device, strip_rows {routes['device'].strip_rows}, the same bytes:")
    for a in routes:
        print(line(f'PngEncoder(assemble="{a}").encode, {F} stills (host clock)', t[f"encode_{a}"]))
        print(line(f'PngEncoder(assemble="{a}").encode_apng, one animation (host clock)', t[f"apng_{a}"]))
    print(line(f"sp_crc32_rows over the {F} streams, two kernels (device events)", t["crc_rows"]))
    print(line("sp_png_wrap, stills: chunks, CRC-32, the streams into the files, four kernels (device events)", t["wrap_stills"]))
    print(line("sp_png_wrap, one animation, four kernels (device events)", t["wrap_apng"]))
    print(f"  host route over device route, medians: encode {med(t['encode_host']) / med(t['encode_device']):.2f} x, "
          f"encode_apng {med(t['apng_host']) / med(t['apng_device']):.2f} x")
    within = [r for r in STRIP_ROWS if sizes[r] <= 1.01 * sizes["one"]]
    best = min(within, key=lambda r: med(t[f"encode{r}"])) if within else None
    print(f"strip heights within 1 % of one strip per frame: {within}; the fastest of them: {best}")


with torch.no_grad():
    main()
