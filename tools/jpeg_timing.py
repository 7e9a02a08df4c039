#!/usr/bin/env python3
"""What a compressed video file costs, per video of 14 frames of 576 x 1024 (profiles/jpeg_timing.txt):

  * the GPU route: sp_jpeg_dct_quant_u8, sp_jpeg_entropy, the device-to-host copy of the lengths and of the used bytes
    (JpegEncoder.collect), and JpegEncoder.encode as a whole (host clock around a call that ends synchronised);
  * the route without the kernels: the device-to-host copy of the uint8 frames, then Pillow's encode of every frame on the
    host at the same quality (one thread: Pillow's JPEG encoder is single-threaded and the frames are encoded in turn);
  * the compressed bytes per video of both.

Inputs: a smooth two-sinusoid colour field plus sigma = 8 noise, and the output of the tiny random-init decoder enlarged
eight times (nearest neighbour).  Device events around the device work, a host clock around what ends on the host; NWARM
warm-up rounds, then the median, minimum and maximum of NREP rounds, the routes alternating round by round.
usage: jpeg_timing.py   (environment: NREP=20 NWARM=3 QUALITY=90)"""
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
from vdpp_amd.models.image_io import JpegEncoder
from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict

NREP, NWARM = int(os.environ.get("NREP", 20)), int(os.environ.get("NWARM", 3))
QUALITY = int(os.environ.get("QUALITY", 90))
F, H, W = 14, 576, 1024
dev = torch.device("cuda:0")


def scene(seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((F, H, W, 3), dtype=np.float32)
    for f in range(F):
        for c in range(3):
            out[f, :, :, c] = (128 + 70 * np.sin(2 * np.pi * (x / (370.0 + 90 * c) + 0.13 * f))
                               + 45 * np.sin(2 * np.pi * (y / (230.0 + 50 * c) + x / 910.0 - 0.07 * f * (c + 1))))
    return np.clip(np.rint(out + rng.normal(0, 8, out.shape)), 0, 255).astype(np.uint8)


def decoder_output():
    cfg = VAEDecoderConfig.tiny(64)
    dec = TemporalDecoderHIP(cfg, random_state_dict(cfg, seed=0), dev)
    lat = (torch.randn((1, 4, F, H // 64, W // 64), generator=torch.Generator().manual_seed(1)) * 0.8).half().to(dev)
    small = dec.decode_latents_uint8(lat, F, decode_chunk_size=F)[0]                  # (F, H/8, W/8, 3)
    return small.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).contiguous()


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
        Image.fromarray(f).save(buf, format="JPEG", quality=QUALITY, subsampling=2)
        files.append(buf.getvalue())
    return files


def line(name, t):
    t = sorted(t)
    return f"  {name}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f})"


def measure(name, frames):
    enc = JpegEncoder(dev, H, W, quality=QUALITY)
    n = frames.shape[0]
    coef = enc._buf("coef", (n, enc.mcu_rows, enc.mcu_cols, 6, 64), torch.int16)
    out = enc._buf("stream", (n, enc.cap), torch.uint8)
    lens = enc._buf("len", (n,), torch.int32)
    ws = enc._buf("ws", (ops.jpeg_entropy_ws_bytes(n, enc.mcu_rows, enc.mcu_cols, enc.restart_mcus),), torch.uint8)
    keys = ("dct", "entropy", "copy", "encode", "raw_copy", "pillow")
    t = {k: [] for k in keys}
    for it in range(NWARM + NREP):
        r = {}
        r["dct"], _ = device_ms(lambda: ops.jpeg_dct_quant(frames, coef, quality=QUALITY))
        r["entropy"], _ = device_ms(lambda: ops.jpeg_entropy(coef, out, lens, ws, restart_mcus=enc.restart_mcus))
        r["copy"], ours = host_ms(lambda: enc.collect(out, lens))
        r["encode"], again = host_ms(lambda: enc.encode(frames))
        r["raw_copy"], raw = host_ms(lambda: frames.cpu().numpy())
        r["pillow"], theirs = host_ms(lambda: pillow(raw))
        assert ours == again
        if it >= NWARM:
            for k in keys:
                t[k].append(r[k])
    print(f"{name}: {n} frames of {H}x{W}, quality {QUALITY}, restart interval {enc.restart_mcus} MCUs "
          f"({n * enc.mcu_rows * enc.mcu_cols // enc.restart_mcus} intervals)")
    print(line("GPU route: sp_jpeg_dct_quant_u8 (device events)", t["dct"]))
    print(line("GPU route: sp_jpeg_entropy, three kernels (device events)", t["entropy"]))
    print(line("GPU route: lengths, then the used bytes to the host, files put together (host clock)", t["copy"]))
    print(line("GPU route: JpegEncoder.encode, all of the above in one call (host clock)", t["encode"]))
    print(line(f"host route: the uint8 frames to the host, {frames.numel() / 1e6:.1f} MB (host clock)", t["raw_copy"]))
    print(line("host route: Pillow's encode of the frames in turn, 1 thread (host clock)", t["pillow"]))
    med = lambda k: sorted(t[k])[len(t[k]) // 2]
    print(f"  host route over GPU route, medians: {(med('raw_copy') + med('pillow')) / med('encode'):.1f} x")
    print(f"  compressed bytes per video: GPU route {sum(map(len, ours))}, Pillow {sum(map(len, theirs))} "
          f"(stream buffer {n * enc.cap / 1e6:.1f} MB and scratch {ws.numel() / 1e6:.1f} MB reserved on the device)")


with torch.no_grad():
    print(f"device: {torch.cuda.get_device_name(0)}; {NWARM} warm-up rounds, then {NREP} timed rounds per line")
    measure("two-sinusoid field + sigma 8 noise", torch.from_numpy(scene()).to(dev))
    measure("tiny random-init decoder's frames, enlarged 8 x", decoder_output())
