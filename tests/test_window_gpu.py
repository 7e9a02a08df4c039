"""Long videos as overlapping frame windows on the GPU: ``sp_euler_step_windows_f16`` and ``sp_dpmpp2m_step_windows_f16``
against the fp64 statement (``tests/window_model.py``) and, for one window, against the bytes of the single-window kernels; the
refusals; ``StableVideoUNet(window_stride=)`` against the oracle UNet run per window on the CPU and fused by the statement; the
wiring (one window == the unwindowed model, HIP graphs, windows per call, batched CFG) and the generate mode end to end.

Kernel bound, every output: ``|got - model| <= 1 fp16 ulp of the model value + (8 + 2*ceil(W/S)) * 2^-24 * terms``, ``terms`` the
sum of the magnitudes of the update's terms with each window's weighted eps counted as one (``window_model``: for x' of 2M
``|a*x| + |b*c1|*(|c_skip*x| + sum_k |c_out*wn_k*e_k|) + |b*c2*D_prev|``, for D the bracket alone, for Euler
``|x| + |dt/sigma|*(|x| + |c_skip*x| + sum_k |c_out*wn_k*e_k|)``).  It is the single-window kernel's bound
(``test_solver_gpu.py``: half an ulp for the final rounding, the rest for about a dozen fp32 roundings that do not all line up)
with two more roundings for every window that can cover a frame: the rounding of its weight to fp32 and its fmaf, each relative
to a partial sum that the terms bound.  The sigmas are values of the fp32 table, so the kernels hold them exactly."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import solver_model as sm
from tests import window_model as wm
from tests.golden import make_sampler_tail_golden as golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 25


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


_dev, _run = golden._dev, golden.run_tail      # one tail on numpy inputs (shared with the fixture's generator)


def _within(got, want, terms, shape, what):
    err, lim = np.abs(got.astype(np.float64) - want), wm.bound(want, terms, shape[2], shape[3])
    ok = err <= lim                                                  # (a NaN in `got` compares False)
    print(f"{what}: worst ratio to the bound {np.nanmax(err / lim):.3f}")
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} outside the bound, worst ratio {np.nanmax(err / lim):.3f}"


@pytest.mark.parametrize("shape", wm.SHAPES, ids=["even-coverage", "uneven-coverage", "disjoint-windows", "hw15-one-pixel-coverage4"])
@pytest.mark.parametrize("guidance", ["none", "shared", "per-video"])
@pytest.mark.parametrize("ld_eps", [4, 8])
def test_kernels_against_the_fp64_model(ld_eps, guidance, shape):
    """Both tails at a second-order step (sigma = 15.6) and at step 0 (sigma = 700, ``c2 == 0``: NaN in the history channels
    must not be read).  Unrelated eps in the windows of one frame; eps columns past the fourth and the pad of the per-video
    guidance rows (``ld_guidance = W + 3``) hold NaN."""
    w, s = shape[2], shape[3]
    for name, step in wm.kernel_steps().items():
        euler, solver = wm.split_step(step)
        state, ec, eu, g, ld_g = wm.case_inputs(shape, ld_eps, guidance, channels=8, sigma=step["sigma"],
                                                nan_history=name == "first-order")
        x_new, den, terms, d_terms = wm.dpmpp2m_step_windows(state, ec, eu, g, window=w, stride=s, **solver)
        got = _run(state, ec, eu, g, ld_g, shape, step)
        assert np.isfinite(got).all(), f"{name}: a NaN was read (history with c2 == 0, eps padding or guidance padding)"
        _within(got[:, :4], x_new, terms, shape, f"2M {name} x'")
        _within(got[:, 4:], den, d_terms, shape, f"2M {name} D")
        assert np.array_equal(_run(state, ec, eu, g, ld_g, shape, step, in_place=True), got), "out_state is state"
        lat, ec, eu, g, ld_g = wm.case_inputs(shape, ld_eps, guidance, channels=4, sigma=step["sigma"])
        want, terms = wm.euler_step_windows(lat, ec, eu, g, window=w, stride=s, **euler)
        got = _run(lat, ec, eu, g, ld_g, shape, step)
        _within(got, want, terms, shape, f"Euler {name}")
        assert np.array_equal(_run(lat, ec, eu, g, ld_g, shape, step, in_place=True), got), "out is the latent"


@pytest.mark.parametrize("hw", [(6, 7), (12, 24)], ids=["hw42-one-pixel-per-thread", "hw288-four-pixels-per-thread"])
@pytest.mark.parametrize("guidance", ["none", "shared", "per-video"])
def test_one_window_gives_the_bytes_of_the_single_window_kernels(guidance, hw):
    """``n_win == 1``: the weight is 1.0 and ``fmaf(1, e_0, 0) == e_0``, so both tails return what ``sp_euler_step_rows_f16``
    and ``sp_dpmpp2m_step_rows_f16`` return, byte for byte, in place and out of place."""
    shape = (2, 5, 5, 3) + hw
    for name, step in wm.kernel_steps().items():
        for channels in (4, 8):
            state, ec, eu, g, ld_g = wm.case_inputs(shape, 8, guidance, channels=channels, sigma=step["sigma"],
                                                    nan_history=name == "first-order")
            want = _run(state, ec, eu, g, ld_g, shape, step, rows_kernel=True)
            assert np.isfinite(want).all()
            for in_place in (False, True):
                got = _run(state, ec, eu, g, ld_g, shape, step, in_place=in_place)
                diff = int((got.view(np.uint16) != want.view(np.uint16)).sum())
                assert diff == 0, f"{name}, {channels} channels, in_place={in_place}: {diff} of {got.size} values differ"


@pytest.mark.parametrize("sampler", ["euler", "2m"])
@pytest.mark.parametrize("entry", ["rows", "windows"])
def test_tails_return_the_recorded_bytes(entry, sampler):
    """``tests/golden/sampler_tails.json``: SHA-256 of what every tail returned at the commit the file names, the last one with
    three separate kernels behind the five entry points (``tests/golden/make_sampler_tail_golden.py``).  The one kernel that
    replaced them returns those bytes, out of place and in place."""
    with open(golden.PATH) as fh:
        rec = json.load(fh)["cases"]
    picked = {cid: case for cid, case in golden.cases().items() if cid.startswith(f"{entry}-{sampler}-")}
    assert len(picked) == {"rows": 12, "windows": 48}[entry] and set(golden.cases()) == set(rec)
    for cid, case in picked.items():
        for in_place in (False, True):
            inputs, output = golden.run(case, in_place=in_place)
            assert inputs == rec[cid]["inputs"], f"{cid}: the fixture is stale (numpy generates other inputs than it was recorded on)"
            assert output == rec[cid]["output"], f"{cid}, in_place={in_place}: other bytes than the recorded kernels returned"


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned-four-pixels-per-thread", "latent-2-bytes-off-one-pixel-per-thread"])
def test_euler_rows_entry_at_four_pixels_per_thread_against_the_fp64_model(misalign):
    """``sp_euler_step_rows_f16`` at H*W = 288 takes the four-pixel form (it had none before the tails shared one kernel) and
    falls back to one pixel per thread when the latent is not 8-byte aligned; both within the kernel bound of one window
    (coverage 1) of the fp64 statement."""
    from vdpp_amd.hip import ops
    shape = (2, 5, 5, 5, 12, 24)
    nb, ft, window, stride, h, w = shape
    for guidance in ("none", "shared", "per-video"):
        for name, step in wm.kernel_steps().items():
            euler, _ = wm.split_step(step)
            lat, ec, eu, g, ld_g = wm.case_inputs(shape, 8, guidance, channels=4, sigma=step["sigma"])
            want, terms = wm.euler_step_windows(lat, ec, eu, g, window=window, stride=stride, **euler)
            st = _dev(lat)
            if misalign:
                buf = torch.empty(st.numel() + 4, dtype=torch.float16, device=DEV)
                buf[1:1 + st.numel()] = st.flatten()
                st = buf[1:1 + st.numel()].view(st.shape)
            assert st.data_ptr() % 8 == (2 if misalign else 0)
            out = torch.full(lat.shape, float("nan"), dtype=torch.float16, device=DEV)
            ops.euler_step(st, _dev(ec), _dev(eu), _dev(g), out, ld_eps=8, b=nb, frames=ft, h=h, w=w, ld_guidance=ld_g, **euler)
            torch.cuda.synchronize()
            _within(out.cpu().numpy(), want, terms, shape, f"Euler rows {guidance} {name}")


def test_euler_rows_entry_refuses_bad_arguments_without_launching():
    from vdpp_amd import hip
    lib = hip.load()
    fn = lib.sp_euler_step_rows_f16
    nb, f, h, w = 1, 2, 4, 4
    n = nb * 4 * f * h * w
    stream = torch.cuda.current_stream().cuda_stream
    eps = torch.zeros(nb * f * h * w, 4, dtype=torch.float16, device=DEV)
    gs = torch.ones(f, dtype=torch.float32, device=DEV)
    buf = torch.full((2 * n,), 7.0, dtype=torch.float16, device=DEV)           # the poison a refused call must leave
    st, out = buf[:n], buf[n:]

    def call(latent=st.data_ptr(), ec=eps.data_ptr(), eu=None, ld_eps=4, g=None, ld_g=0, o=out.data_ptr(), sigma=1.0,
             dims=(nb, f, h, w)):
        return fn(latent, ec, eu, ld_eps, g, ld_g, o, sigma, 0.5, *dims, stream)

    for word, kw in (("null", dict(latent=None)), ("null", dict(ec=None)), ("null", dict(o=None)), ("ld_eps", dict(ld_eps=6)),
                     ("ld_eps", dict(ld_eps=0)), ("sigma", dict(sigma=0.0)), ("sigma", dict(sigma=-1.0)),
                     ("guidance", dict(eu=eps.data_ptr())), ("ld_guidance", dict(eu=eps.data_ptr(), g=gs.data_ptr(), ld_g=f - 1)),
                     ("dims", dict(dims=(nb, 0, h, w))), ("dims", dict(dims=(nb, f, 0, w))), ("dims", dict(dims=(0, f, h, w))),
                     ("overlap", dict(o=st.data_ptr() + 2)), ("overlap", dict(o=st.data_ptr() + 2 * (n - 1))),
                     ("overlap", dict(latent=out.data_ptr(), o=out.data_ptr() - 16))):
        assert call(**kw) == -1 and word in hip.last_error() and fn.__name__ in hip.last_error(), (kw, hip.last_error())
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()), "a refused call wrote"
    assert call() == 0 and call(o=st.data_ptr()) == 0                 # apart, and in place (out == latent)
    torch.cuda.synchronize()
    assert not bool((buf == 7.0).any())


def test_kernels_refuse_bad_arguments_without_launching():
    from vdpp_amd import hip
    lib = hip.load()
    nb, ft, window, stride, h, w = 1, 6, 4, 2, 4, 4
    n_win, hw = 2, h * w
    stream = torch.cuda.current_stream().cuda_stream
    eps = torch.zeros(n_win * nb * window * hw, 4, dtype=torch.float16, device=DEV)
    gs = torch.ones(window, dtype=torch.float32, device=DEV)
    wts = torch.full((n_win, window), 0.5, dtype=torch.float32, device=DEV)
    for channels, fn in ((4, lib.sp_euler_step_windows_f16), (8, lib.sp_dpmpp2m_step_windows_f16)):
        n = nb * channels * ft * hw
        buf = torch.full((2 * n,), 7.0, dtype=torch.float16, device=DEV)           # the poison a refused call must leave
        st, out = buf[:n], buf[n:]

        def call(state=st.data_ptr(), ec=eps.data_ptr(), eu=None, ld_eps=4, g=None, ld_g=0, o=out.data_ptr(), sigma=1.0, a=0.5,
                 c2=0.5, dims=(nb, ft, h, w), plan=(window, stride, n_win), weights=wts.data_ptr()):
            coef = (sigma, 0.5) if channels == 4 else (sigma, a, 0.5, 1.5, c2)
            return fn(state, ec, eu, ld_eps, g, ld_g, o, *coef, *dims, *plan, weights, stream)

        def refused(word, **kw):
            assert call(**kw) == -1 and word in hip.last_error(), (channels, kw, hip.last_error())
            assert fn.__name__ in hip.last_error()

        refused("null", state=None)
        refused("null", ec=None)
        refused("null", o=None)
        refused("null weights", weights=None)
        refused("stride", plan=(window, 0, n_win))
        refused("stride", plan=(window, window + 1, n_win))
        refused("whole number of strides", dims=(nb, ft + 1, h, w))
        refused("whole number of strides", plan=(window, 3, n_win))
        refused("n_win", plan=(window, stride, n_win + 1))
        refused("n_win", plan=(window, stride, 1))
        refused("exceeds", plan=(ft + 2, stride, 1))
        refused("ld_eps", ld_eps=6)
        refused("ld_eps", ld_eps=0)
        refused("sigma", sigma=0.0)
        refused("guidance", eu=eps.data_ptr())
        refused("ld_guidance", eu=eps.data_ptr(), g=gs.data_ptr(), ld_g=window - 1)
        refused("dims", dims=(nb, ft, 0, w))
        refused("dims", dims=(0, ft, h, w))
        refused("overlap", o=st.data_ptr() + 2)
        refused("overlap", o=st.data_ptr() + 2 * (n - 1))
        refused("overlap", state=out.data_ptr(), o=out.data_ptr() - 16)
        if channels == 8:
            refused("a =", a=1.0)
            refused("a =", a=-0.1)
            refused("c2", c2=-0.5)
        torch.cuda.synchronize()
        assert bool((buf == 7.0).all()), "a refused call wrote"
        assert call() == 0 and call(o=st.data_ptr()) == 0                 # apart, and in place
        torch.cuda.synchronize()
        assert not bool((buf == 7.0).any())


# ------------------------------------------------------------------------------------------------ the whole step
def _build(c=64, seed=3):
    from oracle.svd_unet_ref import SVDUNetConfig, SVDUNetRef
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict

    cfg = UNetConfig.tiny(c)
    sd = random_state_dict(cfg, seed=seed, dtype=torch.float16)
    ref = SVDUNetRef(SVDUNetConfig.tiny(c)).eval()
    ref.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return cfg, sd, ref, SVDUNetHIP(cfg, sd, DEV)


def _model(hip, sampler, steps=N_STEPS, **kw):
    from vdpp_amd.models.svd_unet import StableVideoUNet
    return StableVideoUNet(unet=hip, timesteps=StableVideoUNet._default_timestep_schedule(steps), sampler=sampler, **kw)


def _oracle_eps_rows(ref, x32, step, model, emb, img):
    """eps rows of the oracle UNet for one video's window, fed as ``svd_step`` feeds it (``oracle/svd_step_ref.py``)."""
    sigma = model.sigmas[step]
    sample = torch.cat([x32 / ((sigma ** 2 + 1) ** 0.5), img], dim=1).permute(0, 2, 1, 3, 4)
    with torch.no_grad():
        eps = ref(sample=sample, timestep=model.scheduler_timesteps[step], encoder_hidden_states=emb,
                  added_time_ids=torch.tensor([[5.0, 127.0, 0.02]]).half().float(), return_dict=False)[0]
    return eps.permute(0, 1, 3, 4, 2).reshape(-1, 4).numpy()


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
@pytest.mark.parametrize("plan", [(1, 8, 4, 2), (2, 6, 4, 2)], ids=["one-video-3-windows", "two-videos-per-video-guidance"])
def test_step_matches_oracle_unet_per_window_fused_by_the_model(plan, sampler):
    """``StableVideoUNet(window_stride=).forward``, guided, against the oracle UNet run on every window of every video on the CPU
    and fused by ``window_model``, at step 18 of 25 (sigma = 0.68: fp16 resolves the increment) and at the tolerances of
    ``test_solver_gpu.py::test_step_matches_oracle_unet_and_model``: x' (and D) within 2e-2, the increment within 5e-2.  The
    same comparison against "the last window overwrites" misses the 2e-2 on x' -- shown on the CPU statement alone, so a step
    that fused nothing would not pass."""
    nb, ft, window, stride = plan
    h, w, step = 8, 16, 18
    cfg, sd, ref, hip = _build(seed=5)
    model = _model(hip, sampler, window_stride=stride)
    g = torch.Generator().manual_seed(21)
    emb = torch.randn(nb, 1, cfg.cross_attention_dim, generator=g).half()
    img = torch.randn(nb, 4, window, h, w, generator=g).half()
    scales = [3.0, 1.5][:nb]
    cond = model.prepare_conditioning(emb.to(DEV), img.to(DEV), guidance_scale=scales if nb > 1 else scales[0],
                                      num_frames=window)
    assert cond.guidance_ld == (window if nb > 1 else 0)
    gs = np.stack([np.linspace(1.0, s, window) for s in scales]).astype(np.float32)
    sig = model.sigmas.double().tolist()
    x = (torch.randn(nb, 4, ft, h, w, generator=g) * (sig[step] + 1)).half()
    starts, _ = wm.plan(ft, window, stride)

    def rows(e, i_lat):
        return np.concatenate([_oracle_eps_rows(ref, x[i:i + 1, :, s:s + window].float(), step, model, e[i:i + 1].float(),
                                                i_lat[i:i + 1].float()) for s in starts for i in range(nb)])

    eps_c, eps_u = rows(emb, img), rows(torch.zeros_like(emb), torch.zeros_like(img))
    xd = x.double().numpy()
    if sampler == "euler":
        kw = dict(sigma=sig[step], sigma_next=sig[step + 1], window=window, stride=stride)
        want_x, _ = wm.euler_step_windows(x.numpy(), eps_c, eps_u, gs, **kw)
        overwritten, _ = wm.euler_step_windows(x.numpy(), eps_c, eps_u, gs, bug="last_overwrites", **kw)
        got = model(x.to(DEV), step, conditioning=cond).float().cpu().numpy()
        base, want_d = xd, None
    else:
        a, b, c1, c2 = model._solver_coef[step]
        assert c2 > 0
        kw = dict(sigma=sig[step], a=a, b=b, c1=c1, c2=c2, window=window, stride=stride)
        state = torch.cat([x, torch.randn(nb, 4, ft, h, w, generator=g).half()], dim=1)
        want_x, want_d, _, _ = wm.dpmpp2m_step_windows(state.numpy(), eps_c, eps_u, gs, **kw)
        overwritten = wm.dpmpp2m_step_windows(state.numpy(), eps_c, eps_u, gs, bug="last_overwrites", **kw)[0]
        got = model(state.to(DEV), step, conditioning=cond).float().cpu().numpy()
        base = a * xd
    assert got.shape == (nb, model.state_channels, ft, h, w) and np.isfinite(got).all()
    miss = rel_l2(overwritten, want_x)
    assert miss > 2e-2, f"'the last window overwrites' would pass: rel_l2 {miss:.3e}"
    ex = rel_l2(got[:, :4], want_x)
    print(f"{sampler} {plan}: rel_l2 x' {ex:.3e} (last-window-overwrites {miss:.3e})")
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
def _conditioning(cfg, frames, h, w, nb=1, seed=9):
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
def test_one_window_equals_the_unwindowed_model_bit_for_bit(sampler):
    """``F_total == W`` with ``window_stride`` set is one window: the stored-eps route and the window tail give the bytes of the
    unwindowed step (for Euler: of the tail fused into ``conv_out``'s epilogue)."""
    cfg, sd, ref, hip = _build(seed=23)
    plain, windowed = _model(hip, sampler), _model(hip, sampler, window_stride=2)
    frames, h, w = 4, 8, 16
    g, emb, img = _conditioning(cfg, frames, h, w, nb=2)
    for guidance in (None, [3.0, 1.5]):
        for m in (plain, windowed):
            m.set_conditioning(emb, img, guidance_scale=guidance, num_frames=frames)
        for step in (0, 7, N_STEPS - 1):
            state = _state(plain, g, 2, frames, h, w)
            assert torch.equal(windowed(state, step), plain(state, step)), f"guidance {guidance}, step {step}"


def test_window_arguments_and_error_texts():
    from vdpp_amd.models.svd_unet import StableVideoUNet
    cfg, sd, ref, hip = _build(seed=31)
    ts = StableVideoUNet._default_timestep_schedule(N_STEPS)
    with pytest.raises(ValueError, match="window_stride"):
        StableVideoUNet(unet=hip, timesteps=ts, window_stride=0)
    with pytest.raises(ValueError, match="window_weights"):
        StableVideoUNet(unet=hip, timesteps=ts, window_stride=2, window_weights="gauss")
    model = StableVideoUNet(unet=hip, timesteps=ts, window_stride=2)
    assert model.window_stride == 2 and model.window_weights == "triangle" and StableVideoUNet(unet=hip, timesteps=ts).window_stride is None
    g, emb, img = _conditioning(cfg, 4, 8, 16)
    model.set_conditioning(emb, img, guidance_scale=2.0, num_frames=4)
    with pytest.raises(ValueError, match=r"frames_total=7, window=4, stride=2.*6 and 8"):
        model(torch.zeros(1, 4, 7, 8, 16, dtype=torch.float16, device=DEV), 3)
    with pytest.raises(ValueError, match="one window"):
        model(torch.zeros(1, 4, 8, 8, 8, dtype=torch.float16, device=DEV), 3)
    assert model(torch.zeros(1, 4, 8, 8, 16, dtype=torch.float16, device=DEV), 3).shape == (1, 4, 8, 8, 16)
    # without window_stride a longer latent is still refused as before
    plain = StableVideoUNet(unet=hip, timesteps=ts)
    plain.set_conditioning(emb, img, guidance_scale=2.0, num_frames=4)
    with pytest.raises(ValueError, match="do not match the latent"):
        plain(torch.zeros(1, 4, 8, 8, 16, dtype=torch.float16, device=DEV), 3)


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
def test_graph_replay_equals_eager(sampler):
    cfg, sd, ref, hip = _build(seed=19)
    eager, graphed = _model(hip, sampler, window_stride=2), _model(hip, sampler, window_stride=2)
    graphed.enable_graphs()
    window, ft, h, w = 4, 8, 8, 16
    g, emb, img = _conditioning(cfg, window, h, w)
    for m in (eager, graphed):
        m.set_conditioning(emb, img, guidance_scale=2.5, num_frames=window)
    for trial in range(2):                       # the first call captures, the second replays with other data
        for step in (0, 7):
            state = _state(eager, g, 1, ft, h, w)
            assert torch.equal(graphed(state, step), eager(state, step)), f"trial {trial} step {step}"
    graphed.enable_graphs(False)


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
def test_two_windows_per_call_equal_one_window_per_call(sampler):
    """Three windows as calls of 2 + 1 windows (stacked as batch rows, the conditioning rows repeated) against three calls."""
    cfg, sd, ref, hip = _build(seed=29)
    one, two = _model(hip, sampler, window_stride=2), _model(hip, sampler, window_stride=2, windows_per_call=2)
    window, ft, h, w = 4, 8, 8, 16
    g, emb, img = _conditioning(cfg, window, h, w, nb=2)
    state = _state(one, g, 2, ft, h, w)
    for guidance in (None, [3.0, 1.5]):
        conds = [m.prepare_conditioning(emb, img, guidance_scale=guidance, num_frames=window) for m in (one, two)]
        a, b = one(state, 7, conditioning=conds[0]), two(state, 7, conditioning=conds[1])
        print(f"{sampler}, guidance {guidance}: rel_l2 {rel_l2(b, a):.3e}")
        assert torch.equal(a, b), f"guidance {guidance}: rel_l2 {rel_l2(b, a):.3e}"


def test_batched_cfg_equals_sequential_cfg_on_the_solver_path():
    """The relation ``test_unet_gpu.py::test_batched_cfg_equals_sequential_cfg`` holds the unwindowed step to: same kernels on
    the same rows, only GEMM tile scheduling differs -> the new sample within 1e-3 relative L2."""
    cfg, sd, ref, hip = _build(seed=17)
    seq, bat = _model(hip, "dpmpp_2m", window_stride=2), _model(hip, "dpmpp_2m", window_stride=2, batched_cfg=True)
    window, ft, h, w = 4, 8, 8, 16
    g, emb, img = _conditioning(cfg, window, h, w, seed=5)
    for m in (seq, bat):
        m.set_conditioning(emb, img, guidance_scale=3.0, num_frames=window)
    state = _state(seq, g, 1, ft, h, w)
    a, b = seq(state, 7), bat(state, 7)
    assert torch.isfinite(b).all() and rel_l2(b[:, :4].float(), a[:, :4].float()) <= 1e-3


# ------------------------------------------------------------------------------------------------ end to end
def _generate_args(src, out, rendezvous, num_frames=8):
    return ["--backend", "gloo", "--init-method", f"file://{rendezvous}", "--log-level", "WARNING", "--random-init", "--tiny",
            "--input-image", str(src), "--height", "64", "--width", "128", "--num-frames", str(num_frames), "--window-frames", "4",
            "--window-stride", "2", "--total-steps", "4", "--output", str(out)]


def test_generate_mode_with_windows_on_one_and_on_two_ranks(monkeypatch, tmp_path, capsys):
    """``modes.generate --num-frames 8 --window-frames 4 --window-stride 2`` in this process and as two rank processes that
    share the GPU and hand the 8-frame latent over Gloo: the same ``.npy`` and ``.gif`` byte for byte, 8 frames in the GIF; an
    illegal total is a parser error that quotes the nearest legal totals."""
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.modes import generate
    rng = np.random.default_rng(5)
    src = tmp_path / "in.png"
    Image.fromarray(rng.integers(0, 256, (96, 160, 3), dtype=np.uint8)).save(src)
    with pytest.raises(SystemExit) as err:
        generate.parse_args(_generate_args(src, tmp_path / "bad.npy", tmp_path / "rendezvous_bad", num_frames=7))
    assert err.value.code == 2
    text = capsys.readouterr().err
    assert "--num-frames 7" in text and "6 and 8" in text, text
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    for ext in ("npy", "gif"):
        generate.main(_generate_args(src, tmp_path / f"one.{ext}", tmp_path / f"rendezvous_one_{ext}"))
        assert not torch.distributed.is_initialized()
    one = np.load(tmp_path / "one.npy")
    assert one.shape == (8, 64, 128, 3) and one.dtype == np.uint8 and int(one.max()) > int(one.min())
    with Image.open(tmp_path / "one.gif") as gif:
        assert gif.n_frames == 8 and gif.size == (128, 64)
    # two ranks on this GPU, started here as test_solver_gpu.py does (both use device 0); the pairs of the two formats run side
    # by side: four rank processes + this one have the GPU open
    procs = {}
    for ext in ("npy", "gif"):
        for rank in range(2):
            env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0",
                       PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
            procs[ext, rank] = subprocess.Popen([sys.executable, "-m", "vdpp_amd.modes.generate"]
                                                + _generate_args(src, tmp_path / f"two.{ext}", tmp_path / f"rendezvous_two_{ext}"),
                                                env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    logs = {k: p.communicate(timeout=300)[0] for k, p in procs.items()}
    assert all(p.returncode == 0 for p in procs.values()), "\n".join(f"{k}: {log[-3000:]}" for k, log in logs.items())
    for ext in ("npy", "gif"):
        assert (tmp_path / f"two.{ext}").read_bytes() == (tmp_path / f"one.{ext}").read_bytes(), f"two ranks gave another .{ext}"
