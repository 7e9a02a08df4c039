#!/usr/bin/env python3
"""Times of the image front end and of the 8-bit decode at the sizes a request has (profiles/image_io_timing.txt):

  * ImageFrontEnd on a 3000 x 4000 picture already on the device -> 576 x 1024 / CLIP 224 (Lanczos cover-resize, crop, bicubic
    CLIP resize, the two normalised tensors), and the same with the picture coming from host memory;
  * decode_latents_uint8 against decode_latents + frames_to_uint8 for one (1, 4, 14, 72, 128) latent, the two alternating.

Device events around each call, NWARM warm-up calls, then the median, minimum and maximum of NREP calls.
usage: image_io_timing.py [NREP=20] [NWARM=3]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import vdpp_amd  # noqa
from vdpp_amd.models.image_io import ImageFrontEnd, frames_to_uint8
from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict

NREP, NWARM = int(os.environ.get("NREP", 20)), int(os.environ.get("NWARM", 3))
dev = torch.device("cuda:0")


def timed(fns):
    """ms of every call of each fn in fns, the fns alternating."""
    times = [[] for _ in fns]
    for it in range(NWARM + NREP):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= NWARM:
                times[k].append(e0.elapsed_time(e1))
    return times


def line(name, t):
    t = sorted(t)
    return f"{name}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}, {len(t)} calls after {NWARM} warm-up)"


with torch.no_grad():
    host = torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    on_dev = host.to(dev)
    fe = ImageFrontEnd(dev, 576, 1024)
    t_dev, t_host = timed([lambda: fe(on_dev), lambda: fe(host)])
    cfg = VAEDecoderConfig.svd()
    dec = TemporalDecoderHIP(cfg, random_state_dict(cfg, seed=0), dev)
    lat = (torch.randn((1, 4, 14, 72, 128), device=dev) * cfg.scaling_factor).half()
    t_u8, t_f32 = timed([lambda: dec.decode_latents_uint8(lat, 14, decode_chunk_size=14),
                         lambda: frames_to_uint8(dec.decode_latents(lat, 14, decode_chunk_size=14))])
    same = torch.equal(dec.decode_latents_uint8(lat, 14), frames_to_uint8(dec.decode_latents(lat, 14)))
print(f"device: {torch.cuda.get_device_name(0)}")
print(line("ImageFrontEnd 3000x4000 (on the device) -> 576x1024 / 224", t_dev))
print(line("ImageFrontEnd 3000x4000 (from pageable host memory, upload included)", t_host))
print(line("decode_latents_uint8 (1,4,14,72,128), kept result 24.8 MB", t_u8))
print(line("decode_latents + frames_to_uint8 (1,4,14,72,128), fp32 video 99.1 MB in between", t_f32))
print(f"the two decodes give identical bytes: {same}")
