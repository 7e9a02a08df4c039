"""Large frames as overlapping spatial tiles on the GPU: ``sp_euler_step_tiles_f16`` and ``sp_dpmpp2m_step_tiles_f16`` against
the fp64 statement (``tests/tile_model.py``), deterministic and stochastic; for one tile against the bytes of the window, the
stochastic and the single-window entries; the refusals; ``StableVideoUNet(tile_size=, tile_stride=)`` against the oracle UNet run
per patch on the CPU, on that patch's crop of the image latents, and fused by the statement; the wiring (one tile == the
untiled model, HIP graphs, patches per call, batched CFG, seeds across replays) and the generate mode end to end.

Kernel bound, every output (derived in ``tile_model``): ``|got - model| <= 1 fp16 ulp of the model value + (8 + 6*C) * 2^-24 *
terms``, ``C = ceil(Wf/Sf) * ceil(th/sy) * ceil(tw/sx)``, ``terms`` the sum of the magnitudes of the update's terms with each
patch's weighted eps counted as one; a stochastic step adds ``2^-19 * |n*z|`` as in ``test_noise_gpu.py``."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import noise_model as nm
from tests import solver_model as sm
from tests import tile_model as tm
from tests import window_model as wm
from tests.golden import make_sampler_tail_golden as golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 25
GUIDANCE = ("none", "shared", "per-video")


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _dev(t):
    return None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


def _off_by_one_f16(t):
    """A copy of ``t`` that starts 2 bytes off an 8-byte boundary: the tails then take one pixel per thread."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float16, device=DEV)
    buf[1:1 + t.numel()] = t.flatten()
    view = buf[1:1 + t.numel()].view(t.shape)
    assert view.data_ptr() % 8 == 2
    return view


def _record(shape, weights="triangle"):
    from vdpp_amd.hip import ops
    from vdpp_amd.models import tile_plan
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    return ops.TileRecord(tile_plan.plan(h, w, (th, tw), (sy, sx), weights, frames_total=ft, window=wf, window_stride=sf), DEV)


def _run(state, ec, eu, g, ld_g, shape, step, *, in_place=False, misalign=False, noise=None, weights="triangle"):
    """One tiles tail on numpy inputs, numpy out: Euler for a 4-channel ``state``, 2M for 8 channels.  ``step``: a
    ``window_model.kernel_steps`` entry, or with ``noise = (seeds tensor, n or None)`` a ``noise_model.kernel_steps`` entry."""
    from vdpp_amd.hip import ops
    nb = shape[0]
    src = _dev(state)
    if misalign:
        src = _off_by_one_f16(src)
    out = src if in_place else torch.full_like(src, float("nan"))
    if misalign and not in_place:
        out = _off_by_one_f16(out)
    ec, eu, g = _dev(ec), _dev(eu), _dev(g)
    kw = dict(plan=_record(shape, weights), ld_eps=ec.shape[1], ld_guidance=ld_g, sigma=step["sigma"])
    if noise is None:
        euler, solver = wm.split_step(step)
        euler, solver = dict(sigma_next=euler["sigma_next"]), {k: solver[k] for k in ("a", "b", "c1", "c2")}
    else:
        seeds, n = noise
        euler, solver = dict(sigma_next=step["euler"]["sigma_down"]), {k: step["sde"][k] for k in ("a", "b", "c1", "c2")}
        kw.update(seeds=seeds, step=step["step"])
        euler["noise_scale"] = step["euler"]["n"] if n is None else n
        solver["noise_scale"] = step["sde"]["n"] if n is None else n
    if state.shape[1] == 4:
        ops.euler_step_tiles(src, ec, eu, g, out, b=nb, **euler, **kw)
    else:
        ops.dpmpp2m_step_tiles(src, ec, eu, g, out, batch=nb, **solver, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _within(got, want, terms, shape, what, nz=0.0):
    err, lim = np.abs(got.astype(np.float64) - want), tm.bound(want, terms, shape, nz)
    ok = err <= lim                                                  # (a NaN in `got` compares False)
    print(f"{what}: worst ratio to the bound {np.nanmax(err / lim):.3f}")
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} outside the bound, worst ratio {np.nanmax(err / lim):.3f}"


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("shape", tm.SHAPES, ids=tm.SHAPE_IDS)
@pytest.mark.parametrize("guidance", GUIDANCE)
@pytest.mark.parametrize("ld_eps", [4, 8])
def test_kernels_against_the_fp64_model(ld_eps, guidance, shape):
    """Both tails at a second-order step (sigma = 15.6) and at step 0 (sigma = 700, ``c2 == 0``: NaN in the history channels
    must not be read), out of place and in place.  Unrelated eps in the patches of one element; eps columns past the fourth
    and the pad of the per-video guidance rows hold NaN."""
    for name, step in wm.kernel_steps().items():
        euler, solver = wm.split_step(step)
        state, ec, eu, g, ld_g = tm.case_inputs(shape, ld_eps, guidance, channels=8, sigma=step["sigma"],
                                                nan_history=name == "first-order")
        x_new, den, terms, d_terms = tm.dpmpp2m_step_tiles(state, ec, eu, g, shape=shape, **solver)
        got = _run(state, ec, eu, g, ld_g, shape, step)
        assert np.isfinite(got).all(), f"{name}: a NaN was read (history with c2 == 0, eps padding or guidance padding)"
        _within(got[:, :4], x_new, terms, shape, f"2M {name} x'")
        _within(got[:, 4:], den, d_terms, shape, f"2M {name} D")
        assert np.array_equal(_run(state, ec, eu, g, ld_g, shape, step, in_place=True), got), "out_state is state"
        lat, ec, eu, g, ld_g = tm.case_inputs(shape, ld_eps, guidance, channels=4, sigma=step["sigma"])
        want, terms = tm.euler_step_tiles(lat, ec, eu, g, shape=shape, **euler)
        got = _run(lat, ec, eu, g, ld_g, shape, step)
        _within(got, want, terms, shape, f"Euler {name}")
        assert np.array_equal(_run(lat, ec, eu, g, ld_g, shape, step, in_place=True), got), "out is the latent"


@pytest.mark.parametrize("guidance", GUIDANCE)
def test_latent_two_bytes_off_takes_one_pixel_per_thread(guidance):
    """The even-coverage shape would take four pixels per thread; from a view 2 bytes off an 8-byte boundary it takes one, within
    the same bound, and Euler (whose last rounding is one instruction in both forms) with the same bytes."""
    shape = tm.SHAPES[0]
    for name, step in wm.kernel_steps().items():
        euler, solver = wm.split_step(step)
        state, ec, eu, g, ld_g = tm.case_inputs(shape, 8, guidance, channels=8, sigma=step["sigma"], nan_history=name == "first-order")
        x_new, den, terms, d_terms = tm.dpmpp2m_step_tiles(state, ec, eu, g, shape=shape, **solver)
        for in_place in (False, True):
            got = _run(state, ec, eu, g, ld_g, shape, step, misalign=True, in_place=in_place)
            _within(got[:, :4], x_new, terms, shape, f"2M {name} x' (2 bytes off)")
            _within(got[:, 4:], den, d_terms, shape, f"2M {name} D (2 bytes off)")
        lat, ec, eu, g, ld_g = tm.case_inputs(shape, 8, guidance, channels=4, sigma=step["sigma"])
        want, terms = tm.euler_step_tiles(lat, ec, eu, g, shape=shape, **euler)
        got = _run(lat, ec, eu, g, ld_g, shape, step, misalign=True)
        _within(got, want, terms, shape, f"Euler {name} (2 bytes off)")
        assert np.array_equal(got.view(np.uint16), _run(lat, ec, eu, g, ld_g, shape, step).view(np.uint16)), "pixel forms differ"


def _seeds(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("shape", tm.SHAPES, ids=tm.SHAPE_IDS)
@pytest.mark.parametrize("guidance", ["none", "per-video"])
def test_stochastic_steps_against_the_fp64_model(guidance, shape):
    """Euler ancestral and 2M SDE behind tiles: the deterministic statement plus ``n*z`` of the element's address in the LARGE
    latent (``noise_model.step_noise``), within the bound plus ``2^-19 * |n*z|``; D carries no noise."""
    seeds, wshape = _seeds(nm.SEEDS[:shape[0]]), tm.window_shape(shape)
    for name, st in nm.kernel_steps().items():
        state, ec, eu, g, ld_g = tm.case_inputs(shape, 8, guidance, channels=8, sigma=st["sigma"], nan_history=name == "first-order")
        co = {k: st["sde"][k] for k in ("a", "b", "c1", "c2")}
        x_new, den, terms, d_terms = tm.dpmpp2m_step_tiles(state, ec, eu, g, shape=shape, sigma=st["sigma"], **co)
        nz = st["sde"]["n"] * nm.step_noise(nm.SEEDS, wshape, st["step"])
        for in_place in (False, True):
            got = _run(state, ec, eu, g, ld_g, shape, st, noise=(seeds, None), in_place=in_place)
            assert np.isfinite(got).all()
            _within(got[:, :4], x_new + nz, terms + np.abs(nz), shape, f"2M SDE {name} x'", np.abs(nz))
            _within(got[:, 4:], den, d_terms, shape, f"2M SDE {name} D")
        lat, ec, eu, g, ld_g = tm.case_inputs(shape, 8, guidance, channels=4, sigma=st["sigma"])
        want, terms = tm.euler_step_tiles(lat, ec, eu, g, shape=shape, sigma=st["sigma"], sigma_next=st["euler"]["sigma_down"])
        nz = st["euler"]["n"] * nm.step_noise(nm.SEEDS, wshape, st["step"])
        got = _run(lat, ec, eu, g, ld_g, shape, st, noise=(seeds, None))
        _within(got, want + nz, terms + np.abs(nz), shape, f"Euler ancestral {name}", np.abs(nz))


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("hw", [(6, 7), (6, 6), (12, 24)],
                         ids=["hw42-one-pixel", "hw36-four-pixels-across-rows", "hw288-four-pixels"])
@pytest.mark.parametrize("frames", [(5, 3, 2), (5, 5, 5)], ids=["two-windows", "one-window"])
@pytest.mark.parametrize("guidance", GUIDANCE)
def test_one_tile_gives_the_bytes_of_the_window_and_row_kernels(guidance, frames, hw):
    """One tile that is the whole frame: ``wy = wx = {1.0}``, ``(wf*1)*1 == wf`` and the same order of summation, so the tiles
    entries return the bytes of ``sp_*_step_windows_f16``, with one window as well those of ``sp_*_step_rows_f16``, and with
    noise those of ``sp_euler_ancestral_step_f16`` / ``sp_dpmpp2m_sde_step_f16``; in place and out of place."""
    from vdpp_amd.hip import ops
    from vdpp_amd.models import window_plan
    ft, wf, sf = frames
    h, w = hw
    shape = (2, ft, wf, sf, h, w, h, w, h, w)
    wshape = tm.window_shape(shape)
    seeds = _seeds(nm.SEEDS)
    wts = _dev(window_plan.plan(ft, wf, sf).weights)
    noisy = nm.kernel_steps()
    for name, step in wm.kernel_steps().items():
        for channels in (4, 8):
            state, ec, eu, g, ld_g = tm.case_inputs(shape, 8, guidance, channels=channels, sigma=step["sigma"],
                                                    nan_history=name == "first-order")
            wants = [golden.run_tail(state, ec, eu, g, ld_g, wshape, step)]
            if wf == ft:
                wants.append(golden.run_tail(state, ec, eu, g, ld_g, wshape, step, rows_kernel=True))
            for want in wants:
                assert np.isfinite(want).all()
                for in_place in (False, True):
                    got = _run(state, ec, eu, g, ld_g, shape, step, in_place=in_place)
                    diff = int((got.view(np.uint16) != want.view(np.uint16)).sum())
                    assert diff == 0, f"{name}, {channels} channels, in_place={in_place}: {diff} of {got.size} values differ"
            # with noise: against the stochastic entry with the window table
            st = noisy[name]
            out = torch.full(state.shape, float("nan"), dtype=torch.float16, device=DEV)
            kw = dict(ld_eps=8, sigma=st["sigma"], seeds=seeds, step=st["step"], frames_total=ft, h=h, w=w, window=wf, stride=sf,
                      n_win=(ft - wf) // sf + 1, weights=wts, ld_guidance=ld_g)
            if channels == 4:
                ops.euler_ancestral_step(_dev(state), _dev(ec), _dev(eu), _dev(g), out, b=2, sigma_down=st["euler"]["sigma_down"],
                                         noise_scale=st["euler"]["n"], **kw)
            else:
                co = dict(st["sde"])
                ops.dpmpp2m_sde_step(_dev(state), _dev(ec), _dev(eu), _dev(g), out, batch=2, noise_scale=co.pop("n"), **co, **kw)
            torch.cuda.synchronize()
            got = _run(state, ec, eu, g, ld_g, shape, st, noise=(seeds, None))
            assert np.array_equal(got.view(np.uint16), out.cpu().numpy().view(np.uint16)), f"{name}, {channels} channels, with noise"
            quiet = _run(state, ec, eu, g, ld_g, shape, st, noise=(None, 0.0))
            assert not np.array_equal(quiet[:, :4], got[:, :4])


@pytest.mark.parametrize("guidance", ["none", "per-video"])
def test_stochastic_output_does_not_depend_on_the_tiling(guidance):
    """The same large latent with the same eps per ELEMENT, cut as one tile, as disjoint tiles and as overlapping tiles with the
    uniform profile (coverage 1 or 2 per axis: every weight a power of two, so the blend of equal values is exact): the
    same bytes from all three, noise included -- the noise address is the element's in the large latent."""
    nb, ft, h, w = 2, 2, 4, 8
    seeds = _seeds(nm.SEEDS)
    rng = np.random.default_rng(11)
    plain_c = rng.standard_normal((nb, ft, h, w, 4)).astype(np.float16)
    plain_u = rng.standard_normal((nb, ft, h, w, 4)).astype(np.float16) if guidance != "none" else None
    g, ld_g = wm.guidance_rows(guidance, nb, ft)
    for name, st in nm.kernel_steps().items():
        for channels in (4, 8):
            state = (rng.standard_normal((nb, channels, ft, h, w)) * (st["sigma"] + 1.0)).astype(np.float16)
            outs = []
            for th, tw, sy, sx in ((4, 8, 4, 8), (2, 4, 2, 4), (2, 4, 1, 2)):
                shape = (nb, ft, ft, ft, h, w, th, tw, sy, sx)
                rec = _record(shape, "uniform")
                assert all(float(v) in (1.0, 0.5) for t in (rec.plan.wy, rec.plan.wx) for v in t.flatten())

                def tiled(rows):
                    return None if rows is None else np.concatenate(
                        [rows[:, :, y0:y0 + th, x0:x0 + tw].reshape(-1, 4) for *_, y0, x0 in rec.plan.patches()])

                outs.append(_run(state, tiled(plain_c), tiled(plain_u), g, ld_g, shape, st, noise=(seeds, None), weights="uniform"))
            assert np.isfinite(outs[0]).all()
            for other in outs[1:]:
                assert np.array_equal(other.view(np.uint16), outs[0].view(np.uint16)), f"{name}, {channels} channels"


def test_kernels_refuse_bad_arguments_without_launching():
    from vdpp_amd import hip
    lib = hip.load()
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape = (1, 6, 4, 2, 6, 12, 4, 8, 2, 4)
    rec = _record(shape)
    assert lib.sp_tile_plan_size() == ctypes.sizeof(hip.TilePlan)
    stream = torch.cuda.current_stream().cuda_stream
    eps = torch.zeros(tm.n_patch(shape) * nb * wf * th * tw, 4, dtype=torch.float16, device=DEV)
    gs = torch.ones(wf, dtype=torch.float32, device=DEV)
    seeds = _seeds([5])
    for channels, fn in ((4, lib.sp_euler_step_tiles_f16), (8, lib.sp_dpmpp2m_step_tiles_f16)):
        n = nb * channels * ft * h * w
        buf = torch.full((2 * n,), 7.0, dtype=torch.float16, device=DEV)           # the poison a refused call must leave
        st, out = buf[:n], buf[n:]

        def call(state=st.data_ptr(), ec=eps.data_ptr(), eu=None, ld_eps=4, g=None, ld_g=0, o=out.data_ptr(), sigma=1.0, a=0.5,
                 c2=0.5, batch=nb, n_scale=0.0, sd=None, null_plan=False, **plan):
            d = hip.TilePlan.from_buffer_copy(rec.desc)
            for k, v in plan.items():
                setattr(d, k, v)
            coef = (sigma, 0.5) if channels == 4 else (sigma, a, 0.5, 1.5, c2)
            return fn(None if null_plan else ctypes.byref(d), state, ec, eu, ld_eps, g, ld_g, o, *coef, batch, n_scale, sd, 3, stream)

        def refused(word, **kw):
            assert call(**kw) == -1 and word in hip.last_error(), (channels, kw, hip.last_error())
            assert fn.__name__ in hip.last_error()

        refused("null plan", null_plan=True)
        for table in ("wf", "wy", "wx"):
            refused("null table", **{table: None})
        refused("y (total, tile, stride) = (6, 4, 0)", stride_y=0)
        refused("y (total, tile, stride) = (6, 4, 5)", stride_y=5)
        refused("x (total, tile, stride) = (12, 8, 9)", stride_x=9)
        refused("x (total, tile, stride) = (13, 8, 4): the total is not the tile plus a whole number of strides", w=13)
        refused("y (total, tile, stride) = (6, 4, 3): the total is not", stride_y=3)
        refused("y (total, tile, stride) = (6, 7, 2): the tile exceeds", tile_h=7)
        refused("n_ty=3", n_ty=3)
        refused("n_tx=1", n_tx=1)
        refused("stride=0", stride=0)
        refused("whole number of strides", frames_total=7)
        refused("n_win", n_win=3)
        refused("exceeds", window=8, n_win=1)
        refused("dims", h=0)
        refused("dims", tile_w=0)
        refused("dims", batch=0)
        refused("null", state=None)
        refused("null", ec=None)
        refused("null", o=None)
        refused("ld_eps", ld_eps=6)
        refused("sigma", sigma=0.0)
        refused("guidance", eu=eps.data_ptr())
        refused("ld_guidance", eu=eps.data_ptr(), g=gs.data_ptr(), ld_g=wf - 1)
        refused("overlap", o=st.data_ptr() + 2)
        refused("overlap", state=out.data_ptr(), o=out.data_ptr() - 16)
        refused("null seeds", n_scale=0.5)
        refused("noise_scale", n_scale=-1.0, sd=seeds.data_ptr())
        refused("8-byte aligned", n_scale=0.5, sd=seeds.data_ptr() + 4)
        refused("2^34", frames_total=4, window=4, stride=4, n_win=1, h=65536, w=65536, tile_h=65536, tile_w=65536, n_ty=1, n_tx=1,
                o=st.data_ptr())
        if channels == 8:
            refused("a =", a=1.0)
            refused("c2", c2=-0.5)
        torch.cuda.synchronize()
        assert bool((buf == 7.0).all()), "a refused call wrote"
        assert call() == 0 and call(o=st.data_ptr()) == 0 and call(n_scale=0.5, sd=seeds.data_ptr()) == 0
        torch.cuda.synchronize()
        assert not bool((buf == 7.0).any())


# ------------------------------------------------------------------------------------------------ the whole step
@functools.lru_cache(maxsize=None)
def _reference():
    """The tiny configuration, its weights and the oracle UNet on the CPU: once per module."""
    from oracle.svd_unet_ref import SVDUNetConfig, SVDUNetRef
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict
    cfg = UNetConfig.tiny(64)
    sd = random_state_dict(cfg, seed=5, dtype=torch.float16)
    ref = SVDUNetRef(SVDUNetConfig.tiny(64)).eval()
    ref.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return cfg, sd, ref


@functools.lru_cache(maxsize=None)
def _engine():
    """The tiny model's HIP engine: built once per module; every test makes its own ``StableVideoUNet`` around it."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = _reference()
    return SVDUNetHIP(cfg, sd, DEV)


def _model(sampler, steps=N_STEPS, **kw):
    from vdpp_amd.models.svd_unet import StableVideoUNet
    return StableVideoUNet(unet=_engine(), timesteps=StableVideoUNet._default_timestep_schedule(steps), sampler=sampler, **kw)


# name -> (shape (B, F_total, Wf, Sf, H, W, th, tw, sy, sx), guidance scales, window_stride of the model, seed of the inputs)
ORACLE_CASES = {"one-video-two-tiles-two-windows": ((1, 6, 4, 2, 12, 16, 8, 16, 4, 16), [3.0], 2, 21),
                "two-videos-two-tiles-per-video-guidance": ((2, 4, 4, 4, 8, 24, 8, 16, 8, 8), [5.0, 3.0], None, 21)}
ORACLE_STEP = 18
# (the guidance scales of the second case: with the window tests' [3.0, 1.5] "the last tile overwrites" moves x' by 1.98e-2 on the
# oracle's own eps -- a third of the columns lie in the overlap -- which does not clear the 2e-2; with [5.0, 3.0] it is 3.2e-2)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The inputs of one whole-step case and the oracle UNet's eps rows of every patch of every video, on the CPU and shared by
    both samplers: conditional rows on the patch's own crop of the image latents, unconditional rows (zero conditioning), and
    the conditional rows a caller would get who conditions every tile on tile 0's crop.  Eight oracle forwards, and two
    more for the wrong crops."""
    from tests.test_window_gpu import _oracle_eps_rows
    from vdpp_amd.models import tile_plan
    from vdpp_amd.models.svd_unet import StableVideoUNet
    shape, scales, _, seed = ORACLE_CASES[name]
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    cfg, sd, ref = _reference()

    class Schedule:       # what _oracle_eps_rows reads of a model: the sigma table and the continuous timesteps
        pass

    from vdpp_amd.models import euler_schedule
    sched = Schedule()
    sched.sigmas = euler_schedule.karras_sigma_table(len(StableVideoUNet._default_timestep_schedule(N_STEPS)))
    sched.scheduler_timesteps = euler_schedule.continuous_timesteps(sched.sigmas)
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(nb, 1, cfg.cross_attention_dim, generator=g).half()
    img = torch.randn(nb, 4, wf, h, w, generator=g).half()
    sig = sched.sigmas.double().tolist()
    x = (torch.randn(nb, 4, ft, h, w, generator=g) * (sig[ORACLE_STEP] + 1)).half()
    history = torch.randn(nb, 4, ft, h, w, generator=g).half()
    patches = tile_plan.plan(h, w, (th, tw), (sy, sx), frames_total=ft, window=wf, window_stride=sf).patches()

    def rows(e, i_lat):
        return [_oracle_eps_rows(ref, x[i:i + 1, :, f0:f0 + wf, y0:y0 + th, x0:x0 + tw].float(), ORACLE_STEP, sched,
                                 e[i:i + 1].float(), i_lat[i:i + 1, :, :, y0:y0 + th, x0:x0 + tw].float())
                for *_, f0, y0, x0 in patches for i in range(nb)]

    eps_c, eps_u = rows(emb, img), rows(torch.zeros_like(emb), torch.zeros_like(img))
    # the wrong crop changes only the patches that are not at tile (0, 0): run those alone
    wrong = list(eps_c)
    k = 0
    for _, ky, kx, f0, y0, x0 in patches:
        for i in range(nb):
            if (ky, kx) != (0, 0):
                wrong[k] = _oracle_eps_rows(ref, x[i:i + 1, :, f0:f0 + wf, y0:y0 + th, x0:x0 + tw].float(), ORACLE_STEP, sched,
                                            emb[i:i + 1].float(), img[i:i + 1, :, :, 0:th, 0:tw].float())
            k += 1
    gs = np.stack([np.linspace(1.0, s, wf) for s in scales]).astype(np.float32)
    return dict(shape=shape, emb=emb, img=img, x=x, history=history, sig=sig, gs=gs, eps_c=np.concatenate(eps_c),
                eps_u=np.concatenate(eps_u), eps_c_crop0=np.concatenate(wrong))


def oracle_wants(case, sampler, coef=None):
    """``(want x', want D or None, x' of 'the last tile overwrites', x' of 'tile 0's crop everywhere', base of the increment)``
    of the fp64 statement on the oracle's eps rows."""
    shape, sig, x = case["shape"], case["sig"], case["x"]
    if sampler == "euler":
        kw = dict(shape=shape, sigma=sig[ORACLE_STEP], sigma_next=sig[ORACLE_STEP + 1])
        want_x, _ = tm.euler_step_tiles(x.numpy(), case["eps_c"], case["eps_u"], case["gs"], **kw)
        over, _ = tm.euler_step_tiles(x.numpy(), case["eps_c"], case["eps_u"], case["gs"], bug="last_overwrites", **kw)
        crop0, _ = tm.euler_step_tiles(x.numpy(), case["eps_c_crop0"], case["eps_u"], case["gs"], **kw)
        return want_x, None, over, crop0, x.double().numpy()
    a, b, c1, c2 = coef
    kw = dict(shape=shape, sigma=sig[ORACLE_STEP], a=a, b=b, c1=c1, c2=c2)
    state = torch.cat([x, case["history"]], dim=1).numpy()
    want_x, want_d, _, _ = tm.dpmpp2m_step_tiles(state, case["eps_c"], case["eps_u"], case["gs"], **kw)
    over = tm.dpmpp2m_step_tiles(state, case["eps_c"], case["eps_u"], case["gs"], bug="last_overwrites", **kw)[0]
    crop0 = tm.dpmpp2m_step_tiles(state, case["eps_c_crop0"], case["eps_u"], case["gs"], **kw)[0]
    return want_x, want_d, over, crop0, a * x.double().numpy()


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_step_matches_oracle_unet_per_patch_fused_by_the_model(name, sampler):
    """``StableVideoUNet(tile_size=, tile_stride=).forward``, guided, against the oracle UNet run on every patch of every video
    on the CPU -- on that patch's crop of the image latents -- and fused by ``tile_model``, at step 18 of 25 and at the
    tolerances of ``test_window_gpu.py::test_step_matches_oracle_unet_per_window_fused_by_the_model``: x' (and D) within 2e-2,
    the increment within 5e-2.  On the CPU statement alone "the last tile overwrites" and "every tile conditioned on tile 0's
    crop" each miss the 2e-2 on x', so a step that fused nothing or cropped nothing would not pass."""
    case = oracle_case(name)
    shape, scales, window_stride, _ = ORACLE_CASES[name]
    nb, ft, wf, sf, h, w, th, tw, sy, sx = shape
    model = _model(sampler, window_stride=window_stride, tile_size=(th, tw), tile_stride=(sy, sx))
    cond = model.prepare_conditioning(case["emb"].to(DEV), case["img"].to(DEV), guidance_scale=scales if nb > 1 else scales[0],
                                      num_frames=wf)
    assert cond.guidance_ld == (wf if nb > 1 else 0)
    coef = None
    state = case["x"]
    if sampler == "dpmpp_2m":
        coef = model._solver_coef[ORACLE_STEP]
        assert coef[3] > 0
        state = torch.cat([case["x"], case["history"]], dim=1)
    want_x, want_d, over, crop0, base = oracle_wants(case, sampler, coef)
    for what, wrong in (("the last tile overwrites", over), ("tile 0's crop everywhere", crop0)):
        miss = rel_l2(wrong, want_x)
        print(f"{sampler} {name}: '{what}' rel_l2 {miss:.3e}")
        assert miss > 2e-2, f"'{what}' would pass: rel_l2 {miss:.3e}"
    got = model(state.to(DEV), ORACLE_STEP, conditioning=cond).float().cpu().numpy()
    assert got.shape == (nb, model.state_channels, ft, h, w) and np.isfinite(got).all()
    ex = rel_l2(got[:, :4], want_x)
    print(f"{sampler} {name}: rel_l2 x' {ex:.3e}")
    assert ex <= 2e-2, f"x' rel_l2 {ex:.3e}"
    if want_d is not None:
        ed = rel_l2(got[:, 4:], want_d)
        print(f"  D {ed:.3e}")
        assert ed <= 2e-2, f"D rel_l2 {ed:.3e}"
    inc_want = want_x - base
    assert float(sm.fp16_ulp(np.sqrt(np.mean(want_x ** 2)))) <= 0.01 * float(np.sqrt(np.mean(inc_want ** 2)))
    ei = rel_l2(got[:, :4] - base, inc_want)
    print(f"  increment {ei:.3e}")
    assert ei <= 5e-2, f"increment rel_l2 {ei:.3e}"


# ------------------------------------------------------------------------------------------------ wiring
def _conditioning(frames, h, w, nb=1, seed=9):
    cfg = _reference()[0]
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(nb, 1, cfg.cross_attention_dim, generator=g).half().to(DEV)
    img = torch.randn(nb, 4, frames, h, w, generator=g).half().to(DEV)
    return g, emb, img


def _state(model, g, nb, frames, h, w, scale=50.0):
    x = torch.randn(nb, 4, frames, h, w, generator=g) * scale
    if model.state_channels == 8:
        x = torch.cat([x, torch.randn(nb, 4, frames, h, w, generator=g)], dim=1)
    return x.half().to(DEV)


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
def test_one_tile_equals_the_untiled_model_bit_for_bit(sampler):
    """``tile_size`` equal to the latent's size is one tile: the stored-eps route and the tiles tail give the bytes of the
    untiled step (for Euler: of the tail fused into ``conv_out``'s epilogue), guided and not, at steps 0, 7 and 24."""
    frames, h, w = 4, 8, 16
    plain, tiled = _model(sampler), _model(sampler, tile_size=(h, w), tile_stride=(h, w))
    g, emb, img = _conditioning(frames, h, w, nb=2)
    for guidance in (None, [3.0, 1.5]):
        for m in (plain, tiled):
            m.set_conditioning(emb, img, guidance_scale=guidance, num_frames=frames)
        for step in (0, 7, N_STEPS - 1):
            state = _state(plain, g, 2, frames, h, w)
            assert torch.equal(tiled(state, step), plain(state, step)), f"guidance {guidance}, step {step}"


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde"])
def test_whole_frame_tile_equals_the_windowed_model_bit_for_bit(sampler):
    """``window_stride`` with ``tile_size = tile_stride`` = the frame is the windowed model: three windows of 4 frames in a
    latent of 6, one tile each; the tiles tail and the crops that are the whole frame give the bytes of the windows tail (with
    noise: of the stochastic entries with the window table), two videos, guided per video and not, at steps 0 and 7."""
    window, ft, h, w = 4, 6, 8, 16
    windowed, tiled = _model(sampler, window_stride=2), _model(sampler, window_stride=2, tile_size=(h, w), tile_stride=(h, w))
    g, emb, img = _conditioning(window, h, w, nb=2)
    for guidance in (None, [3.0, 1.5]):
        cond = windowed.prepare_conditioning(emb, img, guidance_scale=guidance, num_frames=window, noise_seed=[5, 6])
        for step in (0, 7):
            state = _state(windowed, g, 2, ft, h, w)
            want = windowed(state, step, conditioning=cond)
            assert torch.isfinite(want).all()
            assert torch.equal(tiled(state, step, conditioning=cond), want), f"guidance {guidance}, step {step}"


def test_tile_arguments_and_error_texts():
    from vdpp_amd.models.svd_unet import StableVideoUNet
    hip = _engine()
    ts = StableVideoUNet._default_timestep_schedule(N_STEPS)
    with pytest.raises(ValueError, match="go together"):
        StableVideoUNet(unet=hip, timesteps=ts, tile_size=(8, 16))
    with pytest.raises(ValueError, match="tile_weights"):
        StableVideoUNet(unet=hip, timesteps=ts, tile_size=(8, 16), tile_stride=(8, 8), tile_weights="gauss")
    with pytest.raises(ValueError, match=r"x \(tile=16, stride=17\)"):
        StableVideoUNet(unet=hip, timesteps=ts, tile_size=(8, 16), tile_stride=(8, 17))
    model = StableVideoUNet(unet=hip, timesteps=ts, tile_size=(8, 16), tile_stride=(8, 8))
    assert model.tile_size == (8, 16) and model.tile_stride == (8, 8) and model.tile_weights == "triangle"
    assert StableVideoUNet(unet=hip, timesteps=ts).tile_size is None
    g, emb, img = _conditioning(4, 8, 28)
    model.set_conditioning(emb, img, guidance_scale=2.0, num_frames=4)
    with pytest.raises(ValueError, match=r"x \(total=28, tile=16, stride=8\).*24 and 32"):
        model(torch.zeros(1, 4, 4, 8, 28, dtype=torch.float16, device=DEV), 3)
    with pytest.raises(ValueError, match="do not match the latent"):        # the image latents have the LARGE size
        model(torch.zeros(1, 4, 4, 8, 24, dtype=torch.float16, device=DEV), 3)
    g, emb, img = _conditioning(4, 8, 24)
    model.set_conditioning(emb, img, guidance_scale=2.0, num_frames=4)
    assert model(torch.zeros(1, 4, 4, 8, 24, dtype=torch.float16, device=DEV), 3).shape == (1, 4, 4, 8, 24)
    # without tile_size a conditioning of another size is still refused as before
    plain = StableVideoUNet(unet=hip, timesteps=ts)
    plain.set_conditioning(emb, img[:, :, :, :, :16].contiguous(), guidance_scale=2.0, num_frames=4)
    with pytest.raises(ValueError, match="do not match the latent"):
        plain(torch.zeros(1, 4, 4, 8, 24, dtype=torch.float16, device=DEV), 3)


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m", "euler_a"])
def test_graph_replay_equals_eager(sampler):
    """The first call captures, the second replays with other data; for the stochastic sampler the third replays with other
    SEEDS in the lane's conditioning copy and gives that seed's sample."""
    kw = dict(tile_size=(8, 16), tile_stride=(8, 8))
    eager, graphed = _model(sampler, **kw), _model(sampler, **kw)
    graphed.enable_graphs()
    frames, h, w = 3, 8, 24
    g, emb, img = _conditioning(frames, h, w)
    outs = []
    for seed in (3, 3, 2 ** 63 - 1) if eager.stochastic else (None, None):
        cond = eager.prepare_conditioning(emb, img, guidance_scale=2.5, num_frames=frames, noise_seed=seed)
        for step in (0, 7):
            state = _state(eager, g, 1, frames, h, w)
            want = eager(state, step, conditioning=cond)
            assert torch.equal(graphed(state, step, conditioning=cond), want), f"seed {seed} step {step}"
        outs.append((state, want))
    if eager.stochastic:
        state, want = outs[1]
        other = eager(state, 7, conditioning=eager.prepare_conditioning(emb, img, guidance_scale=2.5, num_frames=frames, noise_seed=4))
        assert not torch.equal(other, want), "two seeds, the same sample"
    graphed.enable_graphs(False)


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m_sde"])
def test_two_patches_per_call_equal_one_patch_per_call(sampler):
    """Three tiles times two frame windows as calls of 2 + 2 + 2 patches (stacked as batch rows, each with its own crop) against six
    calls; two videos, guided per video and unguided."""
    kw = dict(window_stride=2, tile_size=(8, 16), tile_stride=(8, 8))
    one, two = _model(sampler, **kw), _model(sampler, windows_per_call=2, **kw)
    window, ft, h, w = 4, 6, 8, 32
    g, emb, img = _conditioning(window, h, w, nb=2)
    state = _state(one, g, 2, ft, h, w)
    for guidance in (None, [3.0, 1.5]):
        conds = [m.prepare_conditioning(emb, img, guidance_scale=guidance, num_frames=window, noise_seed=[5, 6]) for m in (one, two)]
        a, b = one(state, 7, conditioning=conds[0]), two(state, 7, conditioning=conds[1])
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"guidance {guidance}: rel_l2 {rel_l2(b, a):.3e}"


def test_batched_cfg_equals_sequential_cfg():
    """The relation ``test_window_gpu.py::test_batched_cfg_equals_sequential_cfg_on_the_solver_path`` holds the window step to:
    the new sample within 1e-3 relative L2."""
    kw = dict(tile_size=(8, 16), tile_stride=(8, 8))
    seq, bat = _model("dpmpp_2m", **kw), _model("dpmpp_2m", batched_cfg=True, **kw)
    frames, h, w = 4, 8, 24
    g, emb, img = _conditioning(frames, h, w, seed=5)
    for m in (seq, bat):
        m.set_conditioning(emb, img, guidance_scale=3.0, num_frames=frames)
    state = _state(seq, g, 1, frames, h, w)
    a, b = seq(state, 7), bat(state, 7)
    assert torch.isfinite(b).all() and rel_l2(b[:, :4].float(), a[:, :4].float()) <= 1e-3


# ------------------------------------------------------------------------------------------------ end to end
def _generate_args(src, out, rendezvous, width=192):
    return ["--backend", "gloo", "--init-method", f"file://{rendezvous}", "--log-level", "WARNING", "--random-init", "--tiny",
            "--input-image", str(src), "--height", "64", "--width", str(width), "--num-frames", "3", "--tile-height", "64",
            "--tile-width", "128", "--tile-stride-y", "64", "--tile-stride-x", "64", "--total-steps", "4", "--output", str(out)]


def test_generate_mode_with_tiles_on_one_and_on_two_ranks(monkeypatch, tmp_path, capsys):
    """``modes.generate --height 64 --width 192 --tile-height 64 --tile-width 128 --tile-stride-x 64`` in this process and as two
    rank processes that share the GPU and hand the large latent over Gloo: the same ``.npy`` byte for byte, frames of the total
    size; an illegal total is a parser error that quotes the nearest legal totals."""
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.modes import generate
    rng = np.random.default_rng(5)
    src = tmp_path / "in.png"
    Image.fromarray(rng.integers(0, 256, (96, 288, 3), dtype=np.uint8)).save(src)
    with pytest.raises(SystemExit) as err:
        generate.parse_args(_generate_args(src, tmp_path / "bad.npy", tmp_path / "rendezvous_bad", width=200))
    assert err.value.code == 2
    text = capsys.readouterr().err
    assert "--width 200" in text and "192 and 256" in text, text
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    generate.main(_generate_args(src, tmp_path / "one.npy", tmp_path / "rendezvous_one"))
    assert not torch.distributed.is_initialized()
    one = np.load(tmp_path / "one.npy")
    assert one.shape == (3, 64, 192, 3) and one.dtype == np.uint8 and int(one.max()) > int(one.min())
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, "-m", "vdpp_amd.modes.generate"]
                                      + _generate_args(src, tmp_path / "two.npy", tmp_path / "rendezvous_two"),
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(log[-3000:] for log in logs)
    assert (tmp_path / "two.npy").read_bytes() == (tmp_path / "one.npy").read_bytes(), "two ranks gave another file"
