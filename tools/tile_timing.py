#!/usr/bin/env python3
"""Large frames as overlapping spatial tiles, timed at the benchmark tile: two videos per call, 14 frames, tiles of 72x128 latent
cells, random-init full-width weights, no guidance, sampler dpmpp_2m.  Same box, same process, same engine and weights; the arms
alternate for ROUNDS rounds of STEPS steps each (host clock around a synchronised stretch), as tools/window_timing.py does:

  72x192    one tiled step of the (2,8,14,72,192) state: 2 tiles 64 columns apart, two UNet calls and one
            sp_dpmpp2m_step_tiles_f16, against 2 x the plain step of a (2,8,14,72,128) state
  108x192   one tiled step of the (2,8,14,108,192) state: 2 x 2 tiles 36 rows / 64 columns apart, four UNet calls and one tail,
            against 4 x the plain step

then, with device events around LAUNCHES back-to-back launches, the tiles tail alone against sp_dpmpp2m_step_windows_f16 on
buffers of (nearly) equal bytes, each with the bytes it has to move (counted from the shapes) over its time; and the decode of
the whole large latent by the temporal VAE decoder (random-init full-width, one warm-up, then the median of three).
Nothing is asserted on these numbers.
usage: tile_timing.py [--rounds 5] [--steps 3] [--launches 50] [--commit TEXT] [--out profiles/tile_timing.txt]"""
import argparse, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--commit", default="")
ap.add_argument("--no-decode", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_timing.txt"))
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd.hip import ops
from vdpp_amd.models import tile_plan, window_plan
from vdpp_amd.models.svd_unet import StableVideoUNet

B, F, TH, TW = 2, 14, 72, 128
TOTALS = {"72x192": (72, 192, 72, 64), "108x192": (108, 192, 36, 64)}      # H, W, stride_y, stride_x


def tail_bytes(coverage_sum, pixels, guided=False):
    """Bytes one second-order 2M tail has to move: per pixel of every frame the 8 state planes read and the 8 written, 2 bytes
    each, and one 8-byte eps row (two with guidance) per patch covering it."""
    return B * pixels * 16 * 2 + B * coverage_sum * 8 * (2 if guided else 1)


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    ts = StableVideoUNet._default_timestep_schedule(25)
    plain = StableVideoUNet.from_random_init(ts, seed=0, device=dev, sampler="dpmpp_2m")
    torch.manual_seed(42)
    plain.set_dummy_conditioning(B, F, TH, TW, dev)
    short_state = plain.init_state(torch.randn(B, 4, F, TH, TW, device=dev, dtype=torch.float16) * plain.init_noise_sigma)
    first = 1                                    # steps 1.. : the second-order form of the tails
    tiled, states, plans = {}, {}, {}
    for name, (h, w, sy, sx) in TOTALS.items():
        m = tiled[name] = StableVideoUNet(unet=plain.unet, timesteps=ts, sampler="dpmpp_2m", tile_size=(TH, TW), tile_stride=(sy, sx))
        m.set_conditioning(plain._cond.image_embeddings, torch.randn(B, 4, F, h, w, device=dev, dtype=torch.float16), num_frames=F)
        states[name] = m.init_state(torch.randn(B, 4, F, h, w, device=dev, dtype=torch.float16) * plain.init_noise_sigma)
        plans[name] = tile_plan.plan(h, w, (TH, TW), (sy, sx), frames_total=F)

    def run(arm):
        name, kind = arm
        for s in range(first, first + args.steps):
            if kind == "tiled":
                tiled[name](states[name], s)
            else:
                for _ in range(plans[name].n_patch):
                    plain(short_state, s)

    arms = [(n, k) for n in TOTALS for k in ("tiled", "n x plain")]
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

        # the tails alone on stored eps rows (ld_eps 4, as conv_out stores them): tiles at 108x192, 14 frames, against frame
        # windows of a 72x128 latent with F_total chosen for (nearly) the same bytes
        sigma = plain._sigma_host[first]
        a_, b_, c1, c2 = plain._solver_coef[first]
        coef = dict(ld_eps=4, sigma=sigma, a=a_, b=b_, c1=c1, c2=c2, batch=B)
        kernels = {}
        for name, pl in plans.items():
            rec = ops.TileRecord(pl, dev)
            h, w = TOTALS[name][:2]
            eps = torch.randn(pl.n_patch * B * F * TH * TW, 4, device=dev, dtype=torch.float16)
            out = torch.empty_like(states[name])
            nbytes = tail_bytes(int(pl.coverage().sum()), F * h * w)
            kernels[f"sp_dpmpp2m_step_tiles_f16 {name}"] = (
                lambda rec=rec, eps=eps, out=out, st=states[name]: ops.dpmpp2m_step_tiles(st, eps, None, None, out, plan=rec, **coef),
                nbytes, float(pl.coverage().mean()))
        win, stride = 14, 7
        target = max(v[1] for v in kernels.values())
        ft = win
        while tail_bytes(int(window_plan.plan(ft + stride, win, stride).coverage().sum()) * TH * TW, (ft + stride) * TH * TW) <= target:
            ft += stride
        wpl = window_plan.plan(ft, win, stride)
        wstate = plain.init_state(torch.randn(B, 4, ft, TH, TW, device=dev, dtype=torch.float16))
        weps = torch.randn(wpl.n_win * B * win * TH * TW, 4, device=dev, dtype=torch.float16)
        wout, wts = torch.empty_like(wstate), torch.from_numpy(wpl.weights).to(dev)
        kernels[f"sp_dpmpp2m_step_windows_f16 72x128, F_total {ft}"] = (
            lambda: ops.dpmpp2m_step_windows(wstate, weps, None, None, wout, frames_total=ft, h=TH, w=TW, window=win, stride=stride,
                                             n_win=wpl.n_win, weights=wts, **coef),
            tail_bytes(int(wpl.coverage().sum()) * TH * TW, ft * TH * TW), float(wpl.coverage().mean()))
        kernel_us = {k: [] for k in kernels}
        for fn, _, _ in kernels.values():
            fn()
        torch.cuda.synchronize()
        for r in range(7):                                   # alternating, as the arms above
            for name, (fn, _, _) in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record(); e1.synchronize()
                kernel_us[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)

        decode_ms = {}
        if not args.no_decode:
            from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
            vcfg = VAEDecoderConfig.svd()
            decoder = TemporalDecoderHIP(vcfg, random_state_dict(vcfg, seed=3, device=dev), dev)
            for name, (h, w) in {"72x128": (TH, TW), **{n: v[:2] for n, v in TOTALS.items()}}.items():
                lat = torch.randn(1, 4, F, h, w, device=dev, dtype=torch.float16)
                v = []
                try:
                    for i in range(4):
                        torch.cuda.synchronize()
                        t = time.perf_counter(); decoder.decode_latents_uint8(lat, F, decode_chunk_size=F); torch.cuda.synchronize()
                        v.append((time.perf_counter() - t) * 1e3)
                    decode_ms[name] = (statistics.median(v[1:]), h * 8, w * 8)
                except ops.HipKernelError as err:              # a size an engine refuses is a finding, not a timing
                    decode_ms[name] = (str(err), h * 8, w * 8)

    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lines = [f"device: {torch.cuda.get_device_name(0)}; commit: {commit or 'unknown'}; two videos per call, {F} frames, tiles of {TH}x{TW} "
             f"latent cells, random-init full-width UNet, no guidance, dpmpp_2m, one patch per call, eager launches on one stream",
             f"one warm-up round, then {args.rounds} rounds per arm, alternating; a round = steps {first}..{first + args.steps - 1} of 25, "
             f"host clock around the synchronised stretch, ms per step"]
    med = {a: statistics.median(v) for a, v in times.items()}
    for (name, kind), v in times.items():
        label = f"{name} {'tiled' if kind == 'tiled' else str(plans[name].n_patch) + ' x plain'}"
        lines.append(f"  {label:<18} median {med[(name, kind)]:8.3f} ms  best {min(v):8.3f}  worst {max(v):8.3f}   rounds: "
                     f"{' '.join(f'{t:.2f}' for t in v)}")
    for name in TOTALS:
        lines.append(f"  {name}: tiled against {plans[name].n_patch} x plain, medians: "
                     f"{100 * (med[(name, 'tiled')] / med[(name, 'n x plain')] - 1):+.2f} % per step")
    spread = max((max(v) - min(v)) / statistics.median(v) for v in times.values())
    lines.append(f"  run-to-run spread (max - min over median, the widest arm): {100 * spread:.2f} %")
    lines.append(f"tails alone on stored eps rows (ld_eps 4, second-order step), device events around {args.launches} back-to-back launches, "
                 f"7 rounds alternating; bytes counted from the shapes (16 state planes read and written, one 8-byte eps row per pixel and "
                 f"covering patch); the buffers fit the 256 MiB Infinity Cache, so this is the rate the step sees, not an HBM rate:")
    for name, v in kernel_us.items():
        nbytes, cover = kernels[name][1], kernels[name][2]
        lines.append(f"  {name:<46} median {statistics.median(v):7.1f} us  min {min(v):7.1f}  max {max(v):7.1f}   {nbytes / 1e6:6.2f} MB "
                     f"(mean coverage {cover:.2f}) -> {nbytes / (statistics.median(v) * 1e-6) / 1e12:.2f} TB/s")
    if decode_ms:
        lines.append(f"decode of the whole latent of one video, {F} frames in one chunk, random-init full-width temporal decoder, to uint8 "
                     f"frames; host clock, one warm-up, median of three:")
        for name, (ms, ph, pw) in decode_ms.items():
            lines.append(f"  latent {name:<8} -> {ph}x{pw} px   " + (f"{ms:9.1f} ms" if isinstance(ms, float) else f"refused: {ms}"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
