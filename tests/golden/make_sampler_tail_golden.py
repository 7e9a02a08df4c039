"""Record what the sampler tails return, as SHA-256 digests, so that a later commit can be held to the bytes of an earlier one.

    python -m tests.golden.make_sampler_tail_golden --commit <hash of the checkout> [--out sampler_tails.json]

run on the GPU from the root of a checkout of the commit to record.  It uses only the four ``ops`` wrappers
(``euler_step``, ``dpmpp2m_step``, ``euler_step_windows``, ``dpmpp2m_step_windows``) and ``tests.window_model``, so it runs
unchanged in any commit that has them.  ``sampler_tails.json`` was recorded at the commit it names: the last one with three
separate kernels (``euler_kernel``, ``dpmpp2m_kernel``, ``window_step_kernel``) behind the entry points.
``tests/test_window_gpu.py::test_tails_return_the_recorded_bytes`` recomputes the digests with the functions of this file.

Cases, all out of place (the test also runs them in place):
  rows      ``sp_euler_step_rows_f16`` / ``sp_dpmpp2m_step_rows_f16`` on the inputs of
            ``test_one_window_gives_the_bytes_of_the_single_window_kernels``: (2,5,5,3) with H*W 6x7 and 12x24, the three guidance
            modes, both ``window_model.kernel_steps()``, ``ld_eps`` 8
  windows   ``sp_euler_step_windows_f16`` / ``sp_dpmpp2m_step_windows_f16`` on the inputs of
            ``test_kernels_against_the_fp64_model``: ``window_model.SHAPES``, the three guidance modes, ``ld_eps`` 4 and 8, both steps
Per case two digests: of the inputs (a drift of numpy's generator then reads as "fixture stale", not as a kernel error) and
of the output bytes.
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os

import numpy as np
import torch

from tests import window_model as wm

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "sampler_tails.json")
DEV = "cuda:0"
GUIDANCE = ("none", "shared", "per-video")


def cases():
    """``case id -> (entry, shape, ld_eps, guidance mode, step name, channels)``; 4 channels: Euler, 8: 2M."""
    out = {}
    for hw in ((6, 7), (12, 24)):
        for guidance in GUIDANCE:
            for name in wm.kernel_steps():
                for channels in (4, 8):
                    shape = (2, 5, 5, 3) + hw
                    out[f"rows-{'euler' if channels == 4 else '2m'}-hw{hw[0] * hw[1]}-{guidance}-{name}"] = \
                        ("rows", shape, 8, guidance, name, channels)
    for i, shape in enumerate(wm.SHAPES):
        for guidance in GUIDANCE:
            for ld_eps in (4, 8):
                for name in wm.kernel_steps():
                    for channels in (4, 8):
                        out[f"windows-{'euler' if channels == 4 else '2m'}-shape{i}-{guidance}-ld{ld_eps}-{name}"] = \
                            ("windows", shape, ld_eps, guidance, name, channels)
    return out


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _dev(t):
    return None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


def run_tail(state, eps_c, eps_u, guidance, ld_g, shape, step, *, in_place=False, rows_kernel=False):
    """One tail on numpy inputs, numpy out; Euler for a 4-channel ``state``, 2M for 8 channels.  ``rows_kernel``: the entry
    behind one set of eps rows (the shape must be one window)."""
    from vdpp_amd.hip import ops
    from vdpp_amd.models import window_plan
    nb, ft, window, stride, h, w = shape
    euler, solver = wm.split_step(step)
    st = _dev(state)
    out = st if in_place else torch.full_like(st, float("nan"))
    ec, eu, g = _dev(eps_c), _dev(eps_u), _dev(guidance)
    if rows_kernel:
        assert ft == window
        if state.shape[1] == 4:
            ops.euler_step(st, ec, eu, g, out, ld_eps=ec.shape[1], b=nb, frames=ft, h=h, w=w, ld_guidance=ld_g, **euler)
        else:
            ops.dpmpp2m_step(st, ec, eu, g, out, ld_eps=ec.shape[1], batch=nb, frames=ft, h=h, w=w, ld_guidance=ld_g, **solver)
    else:
        pl = window_plan.plan(ft, window, stride)
        kw = dict(ld_eps=ec.shape[1], frames_total=ft, h=h, w=w, window=window, stride=stride, n_win=pl.n_win,
                  weights=_dev(pl.weights), ld_guidance=ld_g)
        if state.shape[1] == 4:
            ops.euler_step_windows(st, ec, eu, g, out, b=nb, **euler, **kw)
        else:
            ops.dpmpp2m_step_windows(st, ec, eu, g, out, batch=nb, **solver, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run(case, in_place=False):
    """``(digest of the inputs, digest of the output bytes)`` of one case."""
    entry, shape, ld_eps, guidance, name, channels = case
    step = wm.kernel_steps()[name]
    state, ec, eu, g, ld_g = wm.case_inputs(shape, ld_eps, guidance, channels=channels, sigma=step["sigma"],
                                            nan_history=channels == 8 and name == "first-order")
    out = run_tail(state, ec, eu, g, ld_g, shape, step, in_place=in_place, rows_kernel=entry == "rows")
    return _sha(state, ec, eu, g), _sha(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose kernels are being recorded")
    ap.add_argument("--out", default=PATH)
    args = ap.parse_args()
    import vdpp_amd  # noqa: F401  (registers the package directory under its importable name)
    rec = {}
    for cid, case in cases().items():
        inputs, output = run(case)
        rec[cid] = {"inputs": inputs, "output": output}
    with open(args.out, "w") as fh:
        json.dump({"commit": args.commit, "device": torch.cuda.get_device_name(0), "cases": rec}, fh, indent=1)
        fh.write("\n")
    print(f"{len(rec)} cases -> {args.out}")


if __name__ == "__main__":
    main()
