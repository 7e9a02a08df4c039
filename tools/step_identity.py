#!/usr/bin/env python3
"""The bytes of ``StableVideoUNet.forward`` over every step path, one line per case: the case's name and the sha256 of the
output.  Two commits whose listings are equal line for line compute the same steps; the tool uses the public API alone
(``StableVideoUNet(unet=...)``, ``prepare_conditioning``, ``forward``), so the same file runs on either.

Model: ``UNetConfig.tiny(64)``, weights of seed 5, 25 steps, two videos.  Cases: the four samplers x the plan (none: 4 frames
of 8x16; windows: 6 frames as windows of 4, 2 apart; tiles: 8x24 as tiles of 8x16, 8 apart; both: 6 frames of 8x32) x
guidance (none, per video [3.0, 1.5]) x ``batched_cfg`` (where guided) x ``windows_per_call`` 1 / 2 (where there is a plan) x
steps 0, 7 and 24, ``eta = 1``, noise seeds [5, 6]; then one case per sampler replayed from a captured graph.
usage: step_identity.py [--steps 0,7,24] [--no-graphs] [--out FILE]"""
import argparse, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--steps", default="0,7,24")
ap.add_argument("--no-graphs", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd.models.svd_unet import StableVideoUNet
from vdpp_amd.models.unet_hip import SVDUNetHIP
from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict

DEV = torch.device("cuda:0")
NB, N_STEPS = 2, 25
SAMPLERS = ("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde")
# name -> (model keywords, frames of the latent, frames of the conditioning, h, w)
PLANS = {"none": ({}, 4, 4, 8, 16),
         "windows": (dict(window_stride=2), 6, 4, 8, 16),
         "tiles": (dict(tile_size=(8, 16), tile_stride=(8, 8)), 4, 4, 8, 24),
         "both": (dict(window_stride=2, tile_size=(8, 16), tile_stride=(8, 8)), 6, 4, 8, 32)}


def run_case(engine, cfg, sampler, plan, guidance, batched, per_call, steps, graphs=False):
    """``(name, sha256)`` of the outputs of one model at ``steps``; with ``graphs`` of the replay after the capturing call."""
    kw, ft, win, h, w = PLANS[plan]
    model = StableVideoUNet(unet=engine, timesteps=StableVideoUNet._default_timestep_schedule(N_STEPS), sampler=sampler, eta=1.0,
                            batched_cfg=batched, windows_per_call=per_call, **kw)
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(NB, 1, cfg.cross_attention_dim, generator=g).half().to(DEV)
    img = torch.randn(NB, 4, win, h, w, generator=g).half().to(DEV)
    cond = model.prepare_conditioning(emb, img, guidance_scale=guidance, num_frames=win, noise_seed=[5, 6])
    if graphs:
        model.enable_graphs()
    for step in steps:
        x = torch.randn(NB, 4, ft, h, w, generator=g) * (float(model.sigmas[step]) + 1.0)
        if model.state_channels == 8:
            x = torch.cat([x, torch.randn(NB, 4, ft, h, w, generator=g)], dim=1)
        state = x.half().to(DEV)
        out = model(state, step, conditioning=cond)
        if graphs:
            out = model(state, step, conditioning=cond)
        torch.cuda.synchronize()
        name = (f"{sampler} plan={plan} guidance={'per-video' if guidance else 'none'} batched_cfg={int(batched)} "
                f"per_call={per_call} step={step}{' graph' if graphs else ''}")
        yield name, hashlib.sha256(out.cpu().contiguous().numpy().tobytes()).hexdigest()
    if graphs:
        model.enable_graphs(False)


def main():
    torch.cuda.set_device(DEV)
    cfg = UNetConfig.tiny(64)
    engine = SVDUNetHIP(cfg, random_state_dict(cfg, seed=5, dtype=torch.float16), DEV)
    steps = [int(s) for s in args.steps.split(",")]
    lines = []
    for sampler in SAMPLERS:
        for plan in PLANS:
            for guidance, batched in ((None, False), ([3.0, 1.5], False), ([3.0, 1.5], True)):
                for per_call in (1, 2) if plan != "none" else (1,):
                    lines += [f"{n}  {h}" for n, h in run_case(engine, cfg, sampler, plan, guidance, batched, per_call, steps)]
    if not args.no_graphs:
        for sampler in SAMPLERS:
            lines += [f"{n}  {h}" for n, h in run_case(engine, cfg, sampler, "both", [3.0, 1.5], False, 2, steps[-2:-1] or steps,
                                                       graphs=True)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
