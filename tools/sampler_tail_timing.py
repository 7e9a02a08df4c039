#!/usr/bin/env python3
"""The five sampler-tail entry points alone at the benchmark shape, by the method of tools/window_timing.py (device events around
LAUNCHES back-to-back launches, ROUNDS rounds alternating), with builds of the library of two commits loaded into one process:

  sampler_tail_timing.py --lib parent@<hash>=<that commit's libsvdpipe_hip.so> --lib change=<path> [--out FILE]

Two videos, 72x128 latents, 14 frames behind one set of eps rows, F_total = 28 as three windows of 14 frames 7 apart; ld_eps 4 as
conv_out stores them, guidance on (one row per video; sp_euler_step_f16 its one shared row), the second-order step 1 of 25 for 2M.
An entry of a later library may exceed the first library's median by at most the first's own max - min over its rounds."""
import argparse, ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", default=[], metavar="LABEL=PATH")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_tail_timing.txt"))
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd import hip
from vdpp_amd.models import window_plan
from vdpp_amd.models.euler_schedule import karras_sigma_table
from vdpp_amd.models.solver_schedule import dpmpp_2m_coefficients

B, F, FT, WIN, STRIDE, H, W = 2, 14, 28, 14, 7, 72, 128
dev = torch.device("cuda:0")
libs = {label: ctypes.CDLL(path) for label, path in (spec.split("=", 1) for spec in args.lib or ["this build=" + hip.LIB_PATH])}
torch.manual_seed(42)
sig = karras_sigma_table(25)
euler, solver = (float(sig[1]), float(sig[2])), (float(sig[1]), *dpmpp_2m_coefficients(sig)[1])
pl = window_plan.plan(FT, WIN, STRIDE)


def half(*shape):
    return torch.randn(*shape, device=dev, dtype=torch.float16)


lat, state, lat_long, state_long = half(B, 4, F, H, W), half(B, 8, F, H, W), half(B, 4, FT, H, W), half(B, 8, FT, H, W)
outs = {t: torch.empty_like(t) for t in (lat, state, lat_long, state_long)}
out = {t: o.data_ptr() for t, o in outs.items()}
ec, eu = half(B * F * H * W, 4), half(B * F * H * W, 4)
ec_long, eu_long = half(pl.n_win * B * WIN * H * W, 4), half(pl.n_win * B * WIN * H * W, 4)
g = torch.stack([torch.linspace(1.0, s, WIN) for s in (3.0, 2.0)]).to(dev).contiguous()
weights = torch.from_numpy(pl.weights).to(dev)
stream = torch.cuda.current_stream().cuda_stream
short, long_, plan = (ec.data_ptr(), eu.data_ptr(), 4, g.data_ptr()), (ec_long.data_ptr(), eu_long.data_ptr(), 4, g.data_ptr()), \
    (WIN, STRIDE, pl.n_win, weights.data_ptr(), stream)
calls = {
    "sp_euler_step_f16": (lat.data_ptr(), *short, out[lat], *euler, B, F, H, W, stream),
    "sp_euler_step_rows_f16": (lat.data_ptr(), *short, WIN, out[lat], *euler, B, F, H, W, stream),
    "sp_dpmpp2m_step_rows_f16": (state.data_ptr(), *short, WIN, out[state], *solver, B, F, H, W, stream),
    "sp_euler_step_windows_f16": (lat_long.data_ptr(), *long_, WIN, out[lat_long], *euler, B, FT, H, W, *plan),
    "sp_dpmpp2m_step_windows_f16": (state_long.data_ptr(), *long_, WIN, out[state_long], *solver, B, FT, H, W, *plan),
}
fns, us = {}, {}
for label, lib in libs.items():
    for name, argv in calls.items():
        fn = fns[label, name] = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
        assert fn(*argv) == 0, (label, name)                 # warm-up: code object loaded, the launch accepted
        us[label, name] = []
torch.cuda.synchronize()
for r in range(args.rounds):
    for key, fn in fns.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn(*calls[key[1]])
        e1.record(); e1.synchronize()
        us[key].append(e0.elapsed_time(e1) * 1e3 / args.launches)

first = next(iter(libs))
lines = [f"device: {torch.cuda.get_device_name(0)}; libraries: {', '.join(libs)}; two videos, {H}x{W} latents, {F} frames behind one set "
         f"of eps rows, F_total = {FT} as {pl.n_win} windows of {WIN} frames {STRIDE} apart; ld_eps 4, guidance on, second-order 2M step",
         f"device events around {args.launches} back-to-back launches, {args.rounds} rounds alternating between the entries and the "
         f"libraries, one warm-up launch each; us per launch"]
for name in calls:
    for label in libs:
        v, ref = us[label, name], us[first, name]
        over, margin = statistics.median(v) - statistics.median(ref), max(ref) - min(ref)
        lines.append(f"  {name:<28} {label:<16} median {statistics.median(v):6.2f}  min {min(v):6.2f}  max {max(v):6.2f}   rounds: "
                     + " ".join(f"{t:.2f}" for t in v) + ("" if label == first else f"   {over:+.2f} us against {first}, margin "
                                                          f"{margin:.2f}: " + ("within" if over <= margin else "MISSES the margin")))
text = "\n".join(lines) + "\n"
print(text, end="")
with open(args.out, "w") as fh:
    fh.write(text)
