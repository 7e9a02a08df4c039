#!/usr/bin/env python3
"""Same-box A/B of per-video against shared conditioning at the benchmark shape (2,4,14,72,128), fp16, 25-step table:
one micro-batch of two videos per forward, the arms alternating for ROUNDS rounds (the order flips every round).
Arms: ids shared by both videos vs one (fps, motion bucket, noise aug) triple per video; guidance 3.0 for both vs
[3.0, 2.0] (sequential CFG passes, the Euler tail reading one guidance row per video).  Prints ONE JSON line: median ms
per forward of every arm and the per-video / shared ratios.
usage: per_video_ab.py [--rounds 10] [--reps 3] [--step 2]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--step", type=int, default=2)
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd.models.svd_unet import StableVideoUNet

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
model = StableVideoUNet.from_random_init(StableVideoUNet._default_timestep_schedule(25), seed=0, device=dev)
B, F, H, W = 2, 14, 72, 128
g = torch.Generator(device=dev).manual_seed(42)
emb = torch.randn(B, 1, model.unet.cfg.cross_attention_dim, generator=g, device=dev, dtype=torch.float16)
img = torch.randn(B, 4, F, H, W, generator=g, device=dev, dtype=torch.float16)
lat = torch.randn(B, 4, F, H, W, generator=g, device=dev, dtype=torch.float16) * model.init_noise_sigma
per_video = dict(fps=[6, 14], motion_bucket_id=[127, 30], noise_aug_strength=[0.02, 0.25])
arms = {
    "uniform": model.prepare_conditioning(emb, img, num_frames=F),
    "per_video": model.prepare_conditioning(emb, img, num_frames=F, **per_video),
    "guided_uniform": model.prepare_conditioning(emb, img, num_frames=F, guidance_scale=3.0),
    "guided_per_video": model.prepare_conditioning(emb, img, num_frames=F, guidance_scale=[3.0, 2.0]),
}
assert arms["uniform"].added_ids32.dim() == 1 and arms["per_video"].added_ids32.dim() == 2
assert arms["guided_uniform"].guidance_ld == 0 and arms["guided_per_video"].guidance_ld == F

for c in arms.values():                      # warm-up: lazy allocations, position-embedding cache
    model(lat, args.step, conditioning=c)
torch.cuda.synchronize()

times = {k: [] for k in arms}
names = list(arms)
for rnd in range(args.rounds):
    for name in (names if rnd % 2 == 0 else names[::-1]):
        c = arms[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            model(lat, args.step, conditioning=c)
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.reps)

med = {k: statistics.median(v) for k, v in times.items()}
print(json.dumps({
    "shape": [B, 4, F, H, W], "step": args.step, "rounds": args.rounds, "reps": args.reps,
    "device": torch.cuda.get_device_name(0),
    "median_ms_per_forward": {k: round(v, 3) for k, v in med.items()},
    "min_ms_per_forward": {k: round(min(v), 3) for k, v in times.items()},
    "ratio_per_video_ids": round(med["per_video"] / med["uniform"], 4),
    "ratio_per_video_guidance": round(med["guided_per_video"] / med["guided_uniform"], 4),
}))
