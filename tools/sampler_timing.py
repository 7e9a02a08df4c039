#!/usr/bin/env python3
"""One Euler step against one DPM-Solver++(2M) step at the benchmark shape: two videos per call, (2,4,14,72,128) latents,
random-init full-width weights, no guidance (what bench.py's headline runs).  Same box, same process, same engine and weights;
the two samplers alternate for ROUNDS rounds of STEPS steps each (host clock around a synchronised stretch), as
tools/ab_forward.py alternates its arms.  The 2M arm carries the (2,8,14,72,128) state, stores conv_out's four eps channels
and runs sp_dpmpp2m_step_rows_f16 behind them; the Euler arm applies its update in conv_out's epilogue.  The two stochastic
samplers (euler_a, dpmpp_2m_sde; eta = 1) are two more arms of the same alternation: the stored-eps route and the tail kernel
with the step's noise evaluated in registers.  Also timed with device events: the update kernels alone on stored eps rows,
and sp_randn_f16 against torch.randn for the initial latent.
usage: sampler_timing.py [--rounds 7] [--steps 6] [--commit TEXT] [--out profiles/sampler_timing.txt]"""
import argparse, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--frames", type=int, default=14)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_timing.txt"))
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd.hip import ops
from vdpp_amd.models.svd_unet import StableVideoUNet

dev = torch.device("cuda:0")
ts = StableVideoUNet._default_timestep_schedule(25)
euler = StableVideoUNet.from_random_init(ts, seed=0, device=dev)
solver = StableVideoUNet(unet=euler.unet, timesteps=ts, sampler="dpmpp_2m")
B, F, H, W = 2, args.frames, 72, 128
torch.manual_seed(42)
euler.set_dummy_conditioning(B, F, H, W, dev)
solver.set_conditioning(euler._cond.image_embeddings, euler._cond.image_latents, num_frames=F)
noise = torch.randn(B, 4, F, H, W, device=dev, dtype=torch.float16) * euler.init_noise_sigma
euler_a = StableVideoUNet(unet=euler.unet, timesteps=ts, sampler="euler_a")
sde = StableVideoUNet(unet=euler.unet, timesteps=ts, sampler="dpmpp_2m_sde")
for m in (euler_a, sde):
    m.set_conditioning(euler._cond.image_embeddings, euler._cond.image_latents, num_frames=F, noise_seed=[42, 43])
arms = {"euler": (euler, noise), "dpmpp_2m": (solver, solver.init_state(noise)), "euler_a": (euler_a, noise),
        "dpmpp_2m_sde": (sde, sde.init_state(noise))}
first = 1                                    # steps 1.. : the second-order form of the 2M kernel (step 0 is first order)


def run(name):
    model, x = arms[name]
    for s in range(first, first + args.steps):
        x = model(x, s)
    return x


times = {a: [] for a in arms}
with torch.no_grad():
    for a in arms:
        run(a)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for a in arms:
            torch.cuda.synchronize()
            t = time.perf_counter(); run(a); torch.cuda.synchronize()
            times[a].append((time.perf_counter() - t) * 1e3 / args.steps)

    # the update kernels alone, on stored eps rows
    n = B * F * H * W
    eps = torch.randn(n, 64, device=dev, dtype=torch.float16)
    state, out8, out4 = arms["dpmpp_2m"][1], torch.empty_like(arms["dpmpp_2m"][1]), torch.empty_like(noise)
    sigma, sigma_next = euler._sigma_host[first], euler._sigma_host[first + 1]
    a_, b_, c1, c2 = solver._solver_coef[first]
    kernels = {
        "sp_euler_step_rows_f16": lambda: ops.euler_step(noise, eps, None, None, out4, ld_eps=64, sigma=sigma, sigma_next=sigma_next,
                                                         b=B, frames=F, h=H, w=W),
        "sp_dpmpp2m_step_rows_f16": lambda: ops.dpmpp2m_step(state, eps, None, None, out8, ld_eps=64, sigma=sigma, a=a_, b=b_, c1=c1,
                                                             c2=c2, batch=B, frames=F, h=H, w=W),
    }
    seeds = euler_a._cond.noise_seeds
    down, n_e = euler_a._noise_coef[first]
    sa, sb, sc1, sc2, n_s = sde._noise_coef[first]
    rand = torch.empty_like(noise)
    kernels.update({
        "sp_euler_ancestral_step_f16": lambda: ops.euler_ancestral_step(noise, eps, None, None, out4, ld_eps=64, sigma=sigma,
                                                                        sigma_down=down, noise_scale=n_e, seeds=seeds, step=first,
                                                                        b=B, frames_total=F, h=H, w=W),
        "sp_dpmpp2m_sde_step_f16": lambda: ops.dpmpp2m_sde_step(state, eps, None, None, out8, ld_eps=64, sigma=sigma, a=sa, b=sb,
                                                                c1=sc1, c2=sc2, noise_scale=n_s, seeds=seeds, step=first, batch=B,
                                                                frames_total=F, h=H, w=W),
        "sp_randn_f16": lambda: ops.randn(rand, seeds, scale=euler.init_noise_sigma),
        "torch.randn * sigma": lambda: torch.randn(B, 4, F, H, W, device=dev, dtype=torch.float16) * euler.init_noise_sigma,
    })
    kernel_us = {}
    for name, fn in kernels.items():
        fn(); torch.cuda.synchronize()
        samples = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3)
        kernel_us[name] = samples

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
lines = [f"device: {torch.cuda.get_device_name(0)}; commit: {commit or 'unknown'}; latents ({B},4,{F},{H},{W}) fp16, two videos per call, "
         f"random-init full-width UNet, no guidance, eager launches on one stream",
         f"one warm-up round, then {args.rounds} rounds per sampler, alternating; a round = steps {first}..{first + args.steps - 1} of 25, "
         f"host clock around the synchronised stretch, ms per step (= per call of two videos)"]
med = {a: statistics.median(v) for a, v in times.items()}
for a, v in times.items():
    lines.append(f"  {a:<12} median {med[a]:8.3f} ms  best {min(v):8.3f}  worst {max(v):8.3f}   rounds: {' '.join(f'{t:.2f}' for t in v)}")
spread = max((max(v) - min(v)) / statistics.median(v) for v in times.values())
lines.append("  against euler, medians: " + ", ".join(f"{a} {100 * (med[a] / med['euler'] - 1):+.2f} %" for a in arms if a != "euler")
             + f" per step; run-to-run spread (max - min over median, the widest arm): {100 * spread:.2f} %")
lines.append("kernels alone (the updates on stored eps rows, ld_eps 64; the initial latent), device events, 20 launches each:")
for name, v in kernel_us.items():
    lines.append(f"  {name:<28} median {statistics.median(v):7.1f} us  min {min(v):7.1f}  max {max(v):7.1f}")
lines.append(f"arithmetic consequence at the medians: 25 Euler steps = {25 * med['euler'] / 1e3:.3f} s per call; dpmpp_2m steps: "
             + ", ".join(f"{n_} = {n_ * med['dpmpp_2m'] / 1e3:.3f} s" for n_ in (13, 15, 20, 25))
             + "  (step counts are arithmetic only: no claim about image quality on trained weights)")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(text)
