#!/usr/bin/env python3
"""What a picture file costs on its way in, for a 3000 x 4000 and a 1024 x 576 scene at quality 92 without restart markers
(profiles/jpeg_decode_timing.txt):

  * the device route: the header parse and plan on the host, the upload of plan + compressed bytes, sp_jpeg_decode_split,
    sp_jpeg_decode_sync (one round of sync_passes), sp_jpeg_decode_coefficients, sp_jpeg_decode_pixels, each between device
    events, the count of passes, and JpegDecoder.decode as a whole (host clock around a call that ends with the status
    block on the host);
  * the host route in the same run: Pillow's decode of the same file (one thread), then the upload of the pixels.

Input: a smooth two-sinusoid colour field plus sigma = 8 noise.  NWARM warm-up rounds, then the median, minimum and maximum of
NREP rounds, the routes alternating round by round.
usage: jpeg_decode_timing.py [--out FILE]   (default: profiles/jpeg_decode_timing.txt; environment: NREP=20 NWARM=3 QUALITY=92)"""
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
from vdpp_amd.models import image_io

NREP, NWARM = int(os.environ.get("NREP", 20)), int(os.environ.get("NWARM", 3))
QUALITY = int(os.environ.get("QUALITY", 92))
SIZES = ((3000, 4000), (576, 1024))
dev = torch.device("cuda:0")
lines = []


def say(text=""):
    print(text)
    lines.append(text)


def scene(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((h, w, 3), dtype=np.float32)
    for c in range(3):
        out[:, :, c] = (128 + 70 * np.sin(2 * np.pi * (x / (370.0 + 90 * c)))
                        + 45 * np.sin(2 * np.pi * (y / (230.0 + 50 * c) + x / 910.0)))
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


def line(name, t):
    t = sorted(t)
    return f"  {name}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f})"


def measure(h, w):
    buf = io.BytesIO()
    Image.fromarray(scene(h, w)).save(buf, format="JPEG", quality=QUALITY)
    data = buf.getvalue()
    dec = image_io.JpegDecoder(dev)
    k = dec.sync_passes
    keys = ("parse", "upload", "split", "sync", "coef", "pixels", "decode", "pillow", "pixel_upload")
    t = {key: [] for key in keys}
    passes = None
    for it in range(NWARM + NREP):
        r = {}

        def parse():
            info = image_io.parse_jpeg(data)
            return info, ops.jpeg_decode_plan(info.plan_fields(dec.subseq_bits), *info.plan_tables())

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info, plan_host = parse()
        r["parse"] = (time.perf_counter() - t0) * 1e3
        blob = bytearray(plan_host) + data[info.segment_offset:info.segment_offset + info.segment_length]
        r["upload"], up = host_ms(lambda: torch.frombuffer(blob, dtype=torch.uint8).to(dev))
        plan = ops.JpegPlan(plan_host, up[:len(plan_host)])
        ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=dev)
        coef = torch.empty(plan.coef_bytes // 2, dtype=torch.int16, device=dev)
        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        r["split"], _ = device_ms(lambda: ops.jpeg_decode_split(plan, up[len(plan_host):], ws))
        r["sync"], _ = device_ms(lambda: ops.jpeg_decode_sync(plan, ws, 0, k))
        r["coef"], _ = device_ms(lambda: ops.jpeg_decode_coefficients(plan, ws, k - 1, coef))
        r["pixels"], _ = device_ms(lambda: ops.jpeg_decode_pixels(plan, ws, coef, rgb))
        status = ws[:256].view(torch.int32).cpu().tolist()
        assert status[0] == 0 and status[10] == 1, f"one round of {k} passes did not reach the fixed point: {status[:11]}"
        r["decode"], ours = host_ms(lambda: dec.decode(data))
        passes = dec.last_passes
        assert torch.equal(ours, rgb)
        r["pillow"], ref = host_ms(lambda: np.array(Image.open(io.BytesIO(data)).convert("RGB")))
        r["pixel_upload"], theirs = host_ms(lambda: torch.from_numpy(ref).to(dev))
        assert int((ours.int() - theirs.int()).abs().max()) <= 4
        if it >= NWARM:
            for key in keys:
                t[key].append(r[key])
    say(f"{h} x {w}, quality {QUALITY}, no restart markers: file {len(data)} bytes, entropy-coded segment {info.segment_length} bytes, "
        f"{status[5]} subsequences of {dec.subseq_bits} bits, {passes} passes (rounds of {k})")
    say(line("device route: parse_jpeg + sp_jpeg_decode_plan (host clock)", t["parse"]))
    say(line(f"device route: upload of plan + segment, {len(blob) / 1e6:.2f} MB (host clock)", t["upload"]))
    say(line("device route: sp_jpeg_decode_split (device events)", t["split"]))
    say(line(f"device route: sp_jpeg_decode_sync, {k} passes enqueued, {passes} run (device events)", t["sync"]))
    say(line("device route: sp_jpeg_decode_coefficients (device events)", t["coef"]))
    say(line("device route: sp_jpeg_decode_pixels (device events)", t["pixels"]))
    say(line("device route: JpegDecoder.decode, all of the above and the status block read (host clock)", t["decode"]))
    say(line("host route: Pillow's decode, 1 thread (host clock)", t["pillow"]))
    say(line(f"host route: upload of the pixels, {h * w * 3 / 1e6:.1f} MB (host clock)", t["pixel_upload"]))
    med = lambda key: sorted(t[key])[len(t[key]) // 2]                 # noqa: E731
    ratio = (med("pillow") + med("pixel_upload")) / med("decode")
    say(f"  host route over device route, medians: {ratio:.2f} x" + ("" if ratio >= 1 else "  (the device route LOSES at this size)"))
    say()


with torch.no_grad():
    say(f"device: {torch.cuda.get_device_name(0)}; {NWARM} warm-up rounds, then {NREP} timed rounds per line")
    say()
    for hh, ww in SIZES:
        measure(hh, ww)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "jpeg_decode_timing.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
