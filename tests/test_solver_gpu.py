"""DPM-Solver++(2M) on the GPU: ``sp_dpmpp2m_step_rows_f16`` against the fp64 statement (``tests/solver_model.py``) and the
pinned Euler oracle, ``StableVideoUNet(sampler="dpmpp_2m")`` against the oracle UNet, the wiring of the 8-channel state
(hand-over between models, HIP graphs, per-video guidance, the untouched Euler path, the error texts) and the generate mode /
``FrameEmitter`` end to end.

Kernel bound, both output halves: ``|got - model| <= 1 fp16 ulp of the model value + 8 * 2^-24 * (|a*x| + |b*c1*D| +
|b*c2*D_prev|)``.  Half an ulp is the final rounding of an exact result; an fp32 evaluation of the update (three products,
two sums, the two v-prediction constants and the four coefficients rounded to fp32: about a dozen roundings of 2^-24 relative
to one of the three terms each, which do not all line up) stays inside the other half: a factor of two and no more."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import solver_model as sm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 25


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _table():
    from vdpp_amd.models.euler_schedule import continuous_timesteps, karras_sigma_table
    from vdpp_amd.models.solver_schedule import dpmpp_2m_coefficients
    sig32 = karras_sigma_table(N_STEPS)
    return sig32, continuous_timesteps(sig32), dpmpp_2m_coefficients(sig32)


# ------------------------------------------------------------------------------------------------ the kernel
def _run_kernel(state, eps_c, eps_u, guidance, *, ld_guidance, sigma, a, b, c1, c2, in_place=False, misalign=False):
    """numpy in, numpy fp16 (B,8,F,H,W) out.  ``misalign``: the state starts 2 bytes off an 8-byte boundary."""
    from vdpp_amd.hip import ops
    nb, _, f, h, w = state.shape

    def dev(t):
        return None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(DEV)

    st = dev(state)
    if misalign:
        buf = torch.empty(st.numel() + 4, dtype=torch.float16, device=DEV)
        buf[1:1 + st.numel()] = st.flatten()
        st = buf[1:1 + st.numel()].view(st.shape)
        assert st.data_ptr() % 8 == 2
    out = st if in_place else torch.full_like(st, float("nan"))
    ec, eu = dev(eps_c), dev(eps_u)
    ops.dpmpp2m_step(st, ec, eu, dev(guidance), out, ld_eps=ec.shape[1], sigma=sigma, a=a, b=b, c1=c1, c2=c2, batch=nb,
                     frames=f, h=h, w=w, ld_guidance=ld_guidance)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _within(got, want, terms, what):
    err, lim = np.abs(got.astype(np.float64) - want), sm.bound(want, terms)
    ok = err <= lim                                                  # (a NaN in `got` compares False)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} outside the bound, worst ratio {np.nanmax(err / lim):.3f}"


def _guidance_rows(mode, nb, f):
    if mode == "none":
        return None, 0, [None] * nb
    scales = [3.0] * nb if mode == "shared" else [3.0, 2.0][:nb]
    rows = np.stack([np.linspace(1.0, s, f) for s in scales]).astype(np.float32)
    return (rows[0], 0, scales) if mode == "shared" else (rows, f, scales)


def _svd_euler(x, eps_c, eps_u, scales, step, sig32, ts):
    """The oracle's Euler step (fp32) of every video on stored eps rows: ``svd_step`` around a stub UNet that returns them."""
    from oracle.svd_step_ref import svd_step
    nb, _, f, h, w = x.shape
    out = []
    for i in range(nb):
        planes = {k: None if r is None else torch.from_numpy(sm.rows_to_planes(r, nb, f, h, w)[i:i + 1].astype(np.float32))
                  .permute(0, 2, 1, 3, 4) for k, r in (("c", eps_c), ("u", eps_u))}

        def stub(sample, timestep, encoder_hidden_states, added_time_ids, return_dict=False):
            return (planes["c"] if float(encoder_hidden_states.abs().sum()) > 0 else planes["u"],)

        xi = torch.from_numpy(x[i:i + 1].astype(np.float32))
        with torch.no_grad():
            out.append(svd_step(stub, xi, step, sigmas=sig32, timesteps=ts, image_embeddings=torch.ones(1, 1, 4),
                                image_latents=torch.ones_like(xi), added_time_ids=torch.zeros(1, 3),
                                guidance_scale=scales[i], dtype=torch.float32).double().numpy())
    return np.concatenate(out, axis=0)


@pytest.mark.parametrize("shape", [(2, 5, 6, 7), (2, 5, 12, 24)], ids=["hw42-one-pixel-per-thread", "hw288-four-pixels-per-thread"])
@pytest.mark.parametrize("guidance", ["none", "shared", "per-video"])
@pytest.mark.parametrize("ld_eps", [4, 64])
def test_kernel_against_the_fp64_model(ld_eps, guidance, shape):
    """(2,5,6,7) is the odd shape of the Euler kernel's test (H*W = 42: one pixel per thread, two workgroups); H*W = 288 takes
    the four-pixels-per-thread path (three workgroups, the last one ragged), and falls back to one pixel when the state is not
    8-byte aligned.  sigma from 700 (step 0) to 0.002 (step 24) of the 25-step Karras table with its own coefficients."""
    sig32, ts, coef = _table()
    sig = sig32.double().tolist()
    nb, f, h, w = shape
    n = nb * f * h * w
    rng = np.random.default_rng(1000 * ld_eps + 10 * len(guidance) + h)
    g_rows, ld_g, scales = _guidance_rows(guidance, nb, f)

    def eps_rows(grid):
        v = rng.standard_normal((n, ld_eps))
        v = np.round(4.0 * np.clip(v, -1.0, 1.0)) / 4.0 if grid else v
        return v.astype(np.float16)

    def state_for(step, nan_history=False):
        x = rng.standard_normal((nb, 4, f, h, w)) * (sig[step] + 1.0)
        old = np.full_like(x, np.nan) if nan_history else rng.standard_normal((nb, 4, f, h, w))
        return np.concatenate([x, old], axis=1).astype(np.float16)

    # second order: c2 > 0, random eps (the fp16 guidance mix rounds)
    for step in (1, 8, 16, 23):
        a, b, c1, c2 = coef[step]
        assert c2 > 0
        st, ec = state_for(step), eps_rows(False)
        eu = eps_rows(False) if g_rows is not None else None
        kw = dict(ld_guidance=ld_g, sigma=sig[step], a=a, b=b, c1=c1, c2=c2)
        x_new, den, terms = sm.dpmpp2m_step(st, ec, eu, g_rows, sigma=sig[step], a=a, b=b, c1=c1, c2=c2)
        got = _run_kernel(st, ec, eu, g_rows, **kw)
        _within(got[:, :4], x_new, terms, f"step {step} x'")
        _within(got[:, 4:], den, terms, f"step {step} D")
        if step in (8, 23):
            assert np.array_equal(_run_kernel(st, ec, eu, g_rows, in_place=True, **kw), got), "out_state is state"
        if step == 16:
            # (held to the model, not to `got`: the one-pixel and the four-pixel form of the kernel need not round alike --
            # the compiler rounds the fp32 result to fp16 inside the last fma in one of them and behind it in the other)
            off = _run_kernel(st, ec, eu, g_rows, misalign=True, **kw)
            _within(off[:, :4], x_new, terms, f"step {step} x', state 2 bytes off alignment")
            _within(off[:, 4:], den, terms, f"step {step} D, state 2 bytes off alignment")
    # first order: c2 = 0 (step 0, a step in the middle forced to first order, the last step with a = 0), NaN in the history
    # channels, eps on a grid of quarters so that the oracle's fp32 guidance mix equals the fp16 one
    for step in (0, 12, N_STEPS - 1):
        a, b, _, _ = coef[step]
        st, ec = state_for(step, nan_history=True), eps_rows(True)
        eu = eps_rows(True) if g_rows is not None else None
        kw = dict(ld_guidance=ld_g, sigma=sig[step], a=a, b=b, c1=1.0, c2=0.0)
        x_new, den, terms = sm.dpmpp2m_step(st, ec, eu, g_rows, sigma=sig[step], a=a, b=b, c1=1.0, c2=0.0)
        got = _run_kernel(st, ec, eu, g_rows, **kw)
        assert np.isfinite(got).all(), f"step {step}: c2 = 0 read the history channels"
        _within(got[:, :4], x_new, terms, f"step {step} x' (first order)")
        _within(got[:, 4:], den, terms, f"step {step} D (first order)")
        _within(got[:, :4], _svd_euler(st[:, :4], ec, eu, scales, step, sig32, ts), terms, f"step {step} x' against svd_step")
        if step == N_STEPS - 1:
            assert a == 0.0 and np.array_equal(got[:, :4], got[:, 4:]), "sigma' = 0: x' = D"
        assert np.array_equal(_run_kernel(st, ec, eu, g_rows, in_place=True, **kw), got), "out_state is state"


def test_kernel_refuses_bad_arguments_without_launching():
    from vdpp_amd import hip
    lib = hip.load()
    nb, f, h, w = 1, 2, 4, 4
    n = nb * f * h * w
    buf = torch.zeros(2 * 8 * n, dtype=torch.float16, device=DEV)
    st, out = buf[:8 * n], buf[8 * n:]
    eps = torch.zeros(n, 4, dtype=torch.float16, device=DEV)
    gs = torch.ones(f, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(state=st.data_ptr(), ec=eps.data_ptr(), eu=None, ld_eps=4, g=None, ld_g=0, o=out.data_ptr(), sigma=1.0, a=0.5,
             b=0.5, c1=1.5, c2=0.5, dims=(nb, f, h, w)):
        return lib.sp_dpmpp2m_step_rows_f16(state, ec, eu, ld_eps, g, ld_g, o, sigma, a, b, c1, c2, *dims, stream)

    def refused(word, **kw):
        assert call(**kw) == -1 and word in hip.last_error(), (kw, hip.last_error())

    refused("null", state=None)
    refused("null", o=None)
    refused("ld_eps", ld_eps=6)
    refused("ld_eps", ld_eps=0)
    refused("sigma", sigma=0.0)
    refused("sigma", sigma=-1.0)
    refused("a =", a=1.0)
    refused("a =", a=-0.1)
    refused("c2", c2=-0.5)
    refused("guidance", eu=eps.data_ptr())
    refused("ld_guidance", eu=eps.data_ptr(), g=gs.data_ptr(), ld_g=1)
    refused("dims", dims=(nb, 0, h, w))
    refused("overlap", o=st.data_ptr() + 2)
    refused("overlap", o=st.data_ptr() + 2 * (8 * n - 1))
    refused("overlap", state=out.data_ptr(), o=out.data_ptr() - 16)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0, "a refused call wrote"
    assert call() == 0 and call(o=st.data_ptr()) == 0                 # apart, and in place
    torch.cuda.synchronize()


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


def _model(hip, steps=N_STEPS, **kw):
    from vdpp_amd.models.svd_unet import StableVideoUNet
    return StableVideoUNet(unet=hip, timesteps=StableVideoUNet._default_timestep_schedule(steps), sampler="dpmpp_2m", **kw)


def _oracle_eps_rows(ref, x32, step, model, emb, img):
    """eps rows of the oracle UNet, fed as ``svd_step`` feeds it (``oracle/svd_step_ref.py``)."""
    sigma = model.sigmas[step]
    sample = torch.cat([x32 / ((sigma ** 2 + 1) ** 0.5), img], dim=1).permute(0, 2, 1, 3, 4)
    with torch.no_grad():
        eps = ref(sample=sample, timestep=model.scheduler_timesteps[step], encoder_hidden_states=emb,
                  added_time_ids=torch.tensor([[5.0, 127.0, 0.02]]).half().float(), return_dict=False)[0]
    return eps.permute(0, 1, 3, 4, 2).reshape(-1, 4).numpy()


@pytest.mark.parametrize("guidance", [None, 3.0])
def test_step_matches_oracle_unet_and_model(guidance):
    """``StableVideoUNet(sampler="dpmpp_2m").forward`` against the oracle UNet + ``solver_model`` in the tiny configuration of
    ``test_step_matches_oracle_step``: x' and D within its 2e-2; where one fp16 ulp of x' is below 1 % of the increment's rms
    (the late steps) the increment x' - a*x within the 5e-2 the batch-2 oracle test allows an update, while the FIRST-order
    increment of the same inputs misses that by a factor of two or more, so neither an Euler step nor another step's
    coefficients pass."""
    cfg, sd, ref, hip = _build(seed=5)
    model = _model(hip)
    assert model.sampler == "dpmpp_2m" and model.state_channels == 8
    frames, h, w = 4, 8, 16
    g = torch.Generator().manual_seed(21)
    emb = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half()
    img = torch.randn(1, 4, frames, h, w, generator=g).half()
    model.set_conditioning(emb.to(DEV), img.to(DEV), guidance_scale=guidance, num_frames=frames)
    gs = np.linspace(1.0, guidance, frames).astype(np.float32) if guidance else None
    sig = model.sigmas.double().tolist()
    qualified = []
    for step in (1, 12, 18, 23, 24):
        a, b, c1, c2 = model._solver_coef[step]
        x = (torch.randn(1, 4, frames, h, w, generator=g) * (sig[step] + 1)).half()
        eps_c = _oracle_eps_rows(ref, x.float(), step, model, emb.float(), img.float())
        eps_u = _oracle_eps_rows(ref, x.float(), step, model, torch.zeros_like(emb).float(),
                                 torch.zeros_like(img).float()) if guidance else None
        # a history of the estimate's own size, unrelated to it
        probe = np.concatenate([x.numpy(), np.zeros_like(x.numpy())], axis=1)
        d_rms = float(np.sqrt(np.mean(sm.dpmpp2m_step(probe, eps_c, eps_u, gs, sigma=sig[step], a=a, b=b, c1=1.0, c2=0.0)[1] ** 2)))
        old = (torch.randn(1, 4, frames, h, w, generator=g) * d_rms).half()
        state = torch.cat([x, old], dim=1)
        want_x, want_d, _ = sm.dpmpp2m_step(state.numpy(), eps_c, eps_u, gs, sigma=sig[step], a=a, b=b, c1=c1, c2=c2)
        got = model(state.to(DEV), step).float().cpu().numpy()
        assert got.shape == (1, 8, frames, h, w) and np.isfinite(got).all()
        ex, ed = rel_l2(got[:, :4], want_x), rel_l2(got[:, 4:], want_d)
        print(f"guidance {guidance} step {step}: rel_l2 x' {ex:.3e}, D {ed:.3e}")
        assert ex <= 2e-2 and ed <= 2e-2, f"step {step}: rel_l2 x' {ex:.3e}, D {ed:.3e}"
        inc_want = want_x - a * x.double().numpy()
        inc_rms = float(np.sqrt(np.mean(inc_want ** 2)))
        if float(sm.fp16_ulp(np.sqrt(np.mean(want_x ** 2)))) <= 0.01 * inc_rms:
            qualified.append(step)
            ei = rel_l2(got[:, :4] - a * x.double().numpy(), inc_want)
            print(f"  increment rel_l2 {ei:.3e}")
            assert ei <= 5e-2, f"step {step}: increment off, rel_l2={ei:.3e}"
            if c2 > 0:
                first = rel_l2(b * want_d, inc_want)
                assert first >= 2 * 5e-2, f"step {step}: a first-order step would pass (rel_l2={first:.3e})"
    assert set(qualified) >= {18, 23, 24}, f"increment checked at steps {qualified} only"


# ------------------------------------------------------------------------------------------------ wiring
def _conditioning(cfg, frames, h, w, nb=1, seed=9):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(nb, 1, cfg.cross_attention_dim, generator=g).half().to(DEV)
    img = torch.randn(nb, 4, frames, h, w, generator=g).half().to(DEV)
    return g, emb, img


def test_state_handed_between_two_models_continues_bit_identically():
    """Steps 0..5 in one model == steps 0..k there and k+1..5 in a second model built from the same weights that is handed
    nothing but the 8-channel tensor, for every k: the model holds no solver state."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, ref, hip = _build(seed=23)
    first, second = _model(hip, steps=6), _model(SVDUNetHIP(cfg, sd, DEV), steps=6)
    frames, h, w = 3, 8, 16
    g, emb, img = _conditioning(cfg, frames, h, w)
    for m in (first, second):
        m.set_conditioning(emb, img, guidance_scale=2.0, num_frames=frames)
    noise = (torch.randn(1, 4, frames, h, w, generator=g) * first.init_noise_sigma).half().to(DEV)
    states = [first.init_state(noise)]
    assert states[0].shape == (1, 8, frames, h, w) and float(states[0][:, 4:].abs().max()) == 0.0
    assert torch.equal(first.sample_of(states[0]), noise) and first.sample_of(states[0]).data_ptr() == states[0].data_ptr()
    for step in range(6):
        states.append(first(states[-1], step))
    assert torch.isfinite(states[-1]).all()
    assert torch.equal(states[-1][:, :4], states[-1][:, 4:]), "the last step ends on the denoised estimate"
    for k in range(5):
        state = states[k + 1].clone()
        for step in range(k + 1, 6):
            state = second(state, step)
        assert torch.equal(state, states[-1]), f"hand-over after step {k}"
    # and the history is used: without it step 1 gives another sample
    blank = states[1].clone()
    blank[:, 4:] = 0
    assert not torch.equal(first(blank, 1)[:, :4], states[2][:, :4])


def test_graph_replay_equals_eager():
    cfg, sd, ref, hip = _build(seed=19)
    eager, graphed = _model(hip), _model(hip)
    graphed.enable_graphs()
    frames, h, w = 3, 8, 16
    g, emb, img = _conditioning(cfg, frames, h, w)
    for m in (eager, graphed):
        m.set_conditioning(emb, img, guidance_scale=2.5, num_frames=frames)
    for trial in range(2):                       # first call captures, the second replays with other data
        for step in (0, 7):                      # the first-order and the second-order form of the kernel
            state = torch.cat([torch.randn(1, 4, frames, h, w, generator=g) * 50, torch.randn(1, 4, frames, h, w, generator=g)],
                              dim=1).half().to(DEV)
            assert torch.equal(graphed(state, step), eager(state, step)), f"trial {trial} step {step}"
    graphed.enable_graphs(False)


@pytest.mark.parametrize("batched_cfg", [False, True])
def test_pair_with_distinct_guidance_rows_equals_the_single_video_steps(batched_cfg):
    """Two videos with different guidance scales in one call against each video alone, at a late step (where fp16 resolves the
    increment): D and x' - a*x to the 2e-3 of the existing pair-step tests."""
    cfg, sd, ref, hip = _build(seed=45)
    model = _model(hip, batched_cfg=batched_cfg)
    frames, h, w, step = 4, 8, 16, 18
    g, emb, img = _conditioning(cfg, frames, h, w, nb=2)
    a = model._solver_coef[step][0]
    state = torch.cat([torch.randn(2, 4, frames, h, w, generator=g) * float(model.sigmas[step] + 1),
                       torch.randn(2, 4, frames, h, w, generator=g)], dim=1).half().to(DEV)
    scales = [3.0, 1.5]
    pair = model(state, step, conditioning=model.prepare_conditioning(emb, img, guidance_scale=scales, num_frames=frames))
    assert pair.shape == state.shape and torch.isfinite(pair).all()
    for i in range(2):
        one = model.prepare_conditioning(emb[i:i + 1], img[i:i + 1], guidance_scale=scales[i], num_frames=frames)
        single = model(state[i:i + 1].contiguous(), step, conditioning=one)
        x = state[i:i + 1, :4].double()
        e_d = rel_l2(pair[i:i + 1, 4:], single[:, 4:])
        e_i = rel_l2(pair[i:i + 1, :4].double() - a * x, single[:, :4].double() - a * x)
        print(f"video {i}: D {e_d:.3e}, increment {e_i:.3e}")
        assert e_d <= 2e-3 and e_i <= 2e-3, f"video {i}: D {e_d:.3e}, increment {e_i:.3e}"
    assert rel_l2(pair[0:1, 4:], pair[1:2, 4:]) > 1e-2


def test_euler_objects_are_untouched_and_the_error_texts():
    from vdpp_amd.hip import ops
    from vdpp_amd.models.svd_unet import StableVideoUNet

    cfg, sd, ref, hip = _build(seed=31)
    ts = StableVideoUNet._default_timestep_schedule(N_STEPS)
    euler, explicit, solver = StableVideoUNet(unet=hip, timesteps=ts), StableVideoUNet(unet=hip, timesteps=ts, sampler="euler"), _model(hip)
    frames, h, w, step = 3, 16, 24, 11
    g, emb, img = _conditioning(cfg, frames, h, w, seed=12)
    for m in (euler, explicit, solver):
        m.set_conditioning(emb, img, guidance_scale=2.5, num_frames=frames)
    lat = (torch.randn(1, 4, frames, h, w, generator=g) * 30).half().to(DEV)
    assert euler.sampler == "euler" and euler.state_channels == 4
    assert euler.init_state(lat) is lat and euler.sample_of(lat) is lat
    # the two-kernel path test_euler_tail_in_conv_out_epilogue_is_bit_identical holds the fused tail to
    sigma, sigma_next = euler._sigma_host[step], euler._sigma_host[step + 1]
    in_scale = 1.0 / (sigma * sigma + 1.0) ** 0.5
    eps_u = euler._unet_pass(lat, euler._cond.uncond_image_latents, euler._cond.uncond_embeddings, in_scale, step)
    eps_c = euler._unet_pass(lat, euler._cond.image_latents, euler._cond.image_embeddings, in_scale, step)
    want = torch.empty_like(lat)
    ops.euler_step(lat, eps_c, eps_u, euler._cond.guidance32, want, ld_eps=eps_c.shape[1], sigma=sigma, sigma_next=sigma_next, b=1,
                   frames=frames, h=h, w=w)
    assert torch.equal(euler(lat, step), want) and torch.equal(explicit(lat, step), want)
    # error texts
    with pytest.raises(ValueError, match="init_state"):
        solver(lat, step)
    state = solver.init_state(lat)
    with pytest.raises(ValueError, match=r"latent must be \(B, 4, F, H, W\)"):
        euler(state, step)
    with pytest.raises(ValueError, match=r"\(B, 8, F, H, W\)"):
        solver(torch.zeros(1, 6, frames, h, w, dtype=torch.float16, device=DEV), step)
    with pytest.raises(ValueError, match="sampler"):
        StableVideoUNet(unet=hip, timesteps=ts, sampler="heun")
    assert solver(state, step).shape == state.shape


# ------------------------------------------------------------------------------------------------ end to end
def _generate_args(src, out, rendezvous):
    return ["--backend", "gloo", "--init-method", f"file://{rendezvous}", "--log-level", "WARNING", "--random-init", "--tiny",
            "--input-image", str(src), "--height", "64", "--width", "128", "--num-frames", "3", "--sampler", "dpmpp_2m",
            "--total-steps", "6", "--output", str(out)]


def test_generate_mode_with_the_solver_on_one_and_on_two_ranks(monkeypatch, tmp_path):
    """``modes.generate --sampler dpmpp_2m`` in this process and as two rank processes that share the GPU and hand the
    8-channel state over Gloo (a boundary after step 2): the same frames byte for byte."""
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.modes import generate
    rng = np.random.default_rng(5)
    src = tmp_path / "in.png"
    Image.fromarray(rng.integers(0, 256, (96, 160, 3), dtype=np.uint8)).save(src)
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    generate.main(_generate_args(src, tmp_path / "one.npy", tmp_path / "rendezvous_one"))
    assert not torch.distributed.is_initialized()
    one = np.load(tmp_path / "one.npy")
    assert one.shape == (3, 64, 128, 3) and one.dtype == np.uint8 and int(one.max()) > int(one.min())
    # two ranks on this GPU: both use device 0, so the ranks are started here rather than by torchrun (which numbers
    # LOCAL_RANK 0 and 1); two ranks + this process have the GPU open
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, "-m", "vdpp_amd.modes.generate"]
                                      + _generate_args(src, tmp_path / "two.npy", tmp_path / "rendezvous_two"),
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(log[-3000:] for log in logs)
    two = np.load(tmp_path / "two.npy")
    assert two.tobytes() == one.tobytes(), "two ranks gave other frames than one"


def test_frame_emitter_decodes_the_sample_channels_of_the_state():
    from vdpp_amd.models.edge_stages import FrameEmitter
    from vdpp_amd.models.image_io import frames_to_uint8
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    from vdpp_amd.pipeline import LatentSpec, PipelineConfig, PipelineStage
    cfg, sd, ref, hip = _build(seed=0)
    model = _model(hip, steps=2)
    dev = torch.device(DEV)
    vcfg = VAEDecoderConfig.tiny(64)
    decoder = TemporalDecoderHIP(vcfg, random_state_dict(vcfg, seed=19), DEV)
    torch.manual_seed(42)
    model.set_dummy_conditioning(1, 3, 8, 16, dev)
    spec = LatentSpec(shape=torch.Size((1, model.state_channels, 3, 8, 16)), dtype=torch.float16, device=dev)

    def supplier(i):
        g = torch.Generator().manual_seed(1000 + i)
        return model.init_state((torch.randn(1, 4, 3, 8, 16, generator=g) * model.init_noise_sigma).half().to(dev))

    stage = PipelineStage(model, PipelineConfig(total_steps=2, timesteps=[0, 1], world_size=1, rank=0, latent_spec=spec))
    emitter = FrameEmitter(decoder, stage, 3, output="uint8", latent_view=model.sample_of)
    with torch.no_grad():
        out = stage.run_many(2, input_supplier=supplier)
        stage.drain()
        frames = emitter.finish(2)
        assert sorted(frames) == [0, 1]
        for i in range(2):
            assert out[i].shape == (1, 8, 3, 8, 16)
            want = frames_to_uint8(decoder.decode_latents(model.sample_of(out[i]).contiguous(), 3))
            assert frames[i].shape == (1, 3, 64, 128, 3) and torch.equal(frames[i], want)
    with pytest.raises(ValueError, match="latent_view"):
        FrameEmitter(decoder, stage, 3, latent_view="sample")
