#!/usr/bin/env python3
"""Long videos as overlapping frame windows, timed at the benchmark shape: two videos per call, 72x128 latents, F_total = 28
frames as three windows of W = 14, S = 7 apart, random-init full-width weights, no guidance, sampler dpmpp_2m.  Same box, same
process, same engine and weights; the arms alternate for ROUNDS rounds of STEPS steps each (host clock around a synchronised
stretch), as tools/sampler_timing.py alternates its arms:

  windowed   one windowed step of the (2,8,28,72,128) state: three UNet calls and one sp_dpmpp2m_step_windows_f16
  3 x plain  three plain steps of a (2,8,14,72,128) state, the path without window_stride (three UNet calls, three
             sp_dpmpp2m_step_rows_f16): what gluing separate runs together costs per step

and, with device events around LAUNCHES back-to-back launches, the new tail alone against sp_dpmpp2m_step_rows_f16 at 14
frames, each with the bytes it has to move (counted from the shapes below) over its time.
usage: window_timing.py [--rounds 5] [--steps 3] [--launches 50] [--commit TEXT] [--out profiles/window_timing.txt]"""
import argparse, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_timing.txt"))
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd.hip import ops
from vdpp_amd.models import window_plan
from vdpp_amd.models.svd_unet import StableVideoUNet

B, FT, WIN, STRIDE, H, W = 2, 28, 14, 7, 72, 128
HW = H * W


def tail_bytes(frames_total, window, stride, guided=False, history=True):
    """Bytes one 2M tail has to move: per pixel the state planes read (8, or 4 without history) and the 8 written, 2 bytes
    each, and one 8-byte eps row (two with guidance) per window covering the pixel's frame."""
    pl = window_plan.plan(frames_total, window, stride)
    covering = int(pl.coverage().sum())                      # window-frames per video
    planes = B * frames_total * HW * ((8 if history else 4) + 8) * 2
    return planes + B * covering * HW * 8 * (2 if guided else 1)


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    ts = StableVideoUNet._default_timestep_schedule(25)
    plain = StableVideoUNet.from_random_init(ts, seed=0, device=dev, sampler="dpmpp_2m")
    windowed = StableVideoUNet(unet=plain.unet, timesteps=ts, sampler="dpmpp_2m", window_stride=STRIDE)
    torch.manual_seed(42)
    plain.set_dummy_conditioning(B, WIN, H, W, dev)
    windowed.set_conditioning(plain._cond.image_embeddings, plain._cond.image_latents, num_frames=WIN)
    long_state = windowed.init_state(torch.randn(B, 4, FT, H, W, device=dev, dtype=torch.float16) * plain.init_noise_sigma)
    short_state = plain.init_state(torch.randn(B, 4, WIN, H, W, device=dev, dtype=torch.float16) * plain.init_noise_sigma)
    pl = window_plan.plan(FT, WIN, STRIDE)
    first = 1                                    # steps 1.. : the second-order form of the tails

    def run(name):
        for s in range(first, first + args.steps):
            if name == "windowed":
                windowed(long_state, s)
            else:
                for _ in range(pl.n_win):
                    plain(short_state, s)

    arms = ("windowed", "3 x plain")
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

        # the tails alone on stored eps rows (ld_eps 4, as conv_out stores them)
        sigma = plain._sigma_host[first]
        a_, b_, c1, c2 = plain._solver_coef[first]
        eps_long = torch.randn(pl.n_win * B * WIN * HW, 4, device=dev, dtype=torch.float16)
        eps_short = torch.randn(B * WIN * HW, 4, device=dev, dtype=torch.float16)
        out_long, out_short = torch.empty_like(long_state), torch.empty_like(short_state)
        weights = torch.from_numpy(pl.weights).to(dev)
        coef = dict(ld_eps=4, sigma=sigma, a=a_, b=b_, c1=c1, c2=c2, batch=B, h=H, w=W)
        kernels = {
            "sp_dpmpp2m_step_windows_f16": (lambda: ops.dpmpp2m_step_windows(
                long_state, eps_long, None, None, out_long, frames_total=FT, window=WIN, stride=STRIDE, n_win=pl.n_win,
                weights=weights, **coef), tail_bytes(FT, WIN, STRIDE)),
            "sp_dpmpp2m_step_rows_f16": (lambda: ops.dpmpp2m_step(short_state, eps_short, None, None, out_short, frames=WIN,
                                                                 **coef), tail_bytes(WIN, WIN, WIN)),
        }
        kernel_us = {k: [] for k in kernels}
        for name, (fn, _) in kernels.items():
            fn()
        torch.cuda.synchronize()
        for r in range(7):                                   # alternating, as the arms above
            for name, (fn, _) in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record(); e1.synchronize()
                kernel_us[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)

    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lines = [f"device: {torch.cuda.get_device_name(0)}; commit: {commit or 'unknown'}; two videos per call, {H}x{W} latents, F_total = {FT} "
             f"as {pl.n_win} windows of {WIN} frames {STRIDE} apart, random-init full-width UNet, no guidance, dpmpp_2m, eager launches on "
             f"one stream",
             f"one warm-up round, then {args.rounds} rounds per arm, alternating; a round = steps {first}..{first + args.steps - 1} of 25, "
             f"host clock around the synchronised stretch, ms per step"]
    med = {a: statistics.median(v) for a, v in times.items()}
    for a, v in times.items():
        lines.append(f"  {a:<9} median {med[a]:8.3f} ms  best {min(v):8.3f}  worst {max(v):8.3f}   rounds: {' '.join(f'{t:.2f}' for t in v)}")
    spread = max((max(v) - min(v)) / statistics.median(v) for v in times.values())
    lines.append(f"  windowed against 3 x plain, medians: {100 * (med['windowed'] / med['3 x plain'] - 1):+.2f} % per step; run-to-run spread "
                 f"(max - min over median, the wider arm): {100 * spread:.2f} %")
    lines.append(f"tails alone on stored eps rows (ld_eps 4, second-order step), device events around {args.launches} back-to-back launches, "
                 f"7 rounds alternating; bytes counted from the shapes (state planes read and written, one 8-byte eps row per pixel and "
                 f"covering window); the buffers fit the 256 MiB Infinity Cache, so this is the rate the step sees, not an HBM rate:")
    rate = {}
    for name, v in kernel_us.items():
        nbytes = kernels[name][1]
        rate[name] = nbytes / (statistics.median(v) * 1e-6)
        lines.append(f"  {name:<28} median {statistics.median(v):7.1f} us  min {min(v):7.1f}  max {max(v):7.1f}   {nbytes / 1e6:6.2f} MB "
                     f"-> {rate[name] / 1e12:.2f} TB/s")
    ratio = rate["sp_dpmpp2m_step_windows_f16"] / rate["sp_dpmpp2m_step_rows_f16"]
    lines.append(f"  the new tail achieves {100 * ratio:.0f} % of the existing tail's bytes/s measured in this run"
                 + ("" if ratio >= 0.8 else "  (more than 20 % below it: see profiles/window_timing_notes.txt)"))
    lines.append("how to read the tail figures, and the compiler's resource report of the new kernel: profiles/window_timing_notes.txt "
                 "(kept by hand; this file is rewritten by tools/window_timing.py)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
