"""The stochastic samplers on the GPU: the generator word for word against ``tests/noise_model.py``, its normals and the two
stochastic tails (``sp_euler_ancestral_step_f16``, ``sp_dpmpp2m_sde_step_f16``) against the fp64 statement, the bit-for-bit
relations (pixel forms, batch rows, one window, ``n == 0``, ``eta == 0``) and the wiring through ``StableVideoUNet``, HIP graphs
and the generate mode.

Bounds.  The kernel's ``z`` is held to the fp64 model within ``2^-19 * |z|``, sixteen fp32 ulps: the limits the OpenCL profile
sets for ``log`` (3), ``sqrt`` (3), ``sinpi`` / ``cospi`` (4) and one product add to 9.  ``z`` is seen through one rounding to
fp16 of ``scale * z``, which is monotone: the stored value lies between the fp16 roundings of the interval's ends.  A step is
held to the deterministic step's bound (``solver_model.bound`` / ``window_model.bound``, ``terms`` with ``|n*z|``) plus
``2^-19 * |n*z|``."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import noise_model as nm
from tests import window_model as wm

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


def _seeds(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device=DEV)


def _off_by_one_f16(t):
    """A copy of ``t`` that starts 2 bytes off an 8-byte boundary: the tails then take one pixel per thread."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float16, device=DEV)
    buf[1:1 + t.numel()] = t.flatten()
    view = buf[1:1 + t.numel()].view(t.shape)
    assert view.data_ptr() % 8 == 2
    return view


def _run(state, ec, eu, g, ld_g, shape, st, seeds, *, in_place=False, misalign=False, one_window_table=False, n=None):
    """One stochastic tail on numpy inputs, numpy out: Euler ancestral for a 4-channel ``state``, 2M SDE for 8 channels.
    A ``shape`` of one window that is the whole latent goes in unwindowed (``weights=None``) unless ``one_window_table``."""
    from vdpp_amd.hip import ops
    from vdpp_amd.models import window_plan
    nb, ft, window, stride, h, w = shape
    src = _dev(state)
    if misalign:
        src = _off_by_one_f16(src)
    out = src if in_place else torch.full_like(src, float("nan"))
    if misalign and not in_place:
        out = _off_by_one_f16(out)
    ec, eu, g = _dev(ec), _dev(eu), _dev(g)
    kw = dict(ld_eps=ec.shape[1], frames_total=ft, h=h, w=w, ld_guidance=ld_g, seeds=seeds, step=st["step"], sigma=st["sigma"])
    if window != ft or one_window_table:
        pl = window_plan.plan(ft, window, stride)
        kw.update(window=window, stride=stride, n_win=pl.n_win, weights=_dev(pl.weights))
    if state.shape[1] == 4:
        co = dict(st["euler"])
        ops.euler_ancestral_step(src, ec, eu, g, out, b=nb, sigma_down=co["sigma_down"],
                                 noise_scale=co["n"] if n is None else n, **kw)
    else:
        co = dict(st["sde"])
        noise = co.pop("n")
        ops.dpmpp2m_sde_step(src, ec, eu, g, out, batch=nb, noise_scale=noise if n is None else n, **co, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _case(shape, guidance, channels, name, st):
    return wm.case_inputs(shape, 8, guidance, channels=channels, sigma=st["sigma"], nan_history=channels == 8 and name == "first-order")


# ------------------------------------------------------------------------------------------------ the generator
def test_philox_blocks_equal_the_model_word_for_word():
    from vdpp_amd.hip import ops
    n_blocks = 1024
    for seeds in ((0, 2 ** 63 - 1), (42, 0)):
        for step in (0, 7):
            for purpose in (nm.INITIAL, nm.STEP):
                out = torch.full((2, n_blocks, 4), -1, dtype=torch.int32, device=DEV)
                ops.philox_blocks(out, _seeds(seeds), step=step, purpose=purpose)
                got = out.cpu().numpy().view(np.uint32)
                for b, seed in enumerate(seeds):
                    want = nm.blocks(seed, np.arange(n_blocks), step, purpose)
                    assert np.array_equal(got[b], want), f"seed {seed}, step {step}, purpose {purpose}"


def _check_z(got16, z_model, scale, what):
    """``got16`` = fp16(scale * z_kernel) against the model's ``z``: inside the interval of ``2^-19 * |z|``."""
    lo, hi = nm.z_interval_f16(z_model, scale)
    ok = (got16 >= lo) & (got16 <= hi)                               # (a NaN compares False)
    if not ok.all():
        idx = np.argwhere(~ok)[0]
        flat = int(np.ravel_multi_index(tuple(idx[1:]), got16.shape[1:]))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} values outside 2^-19*|z|; first: video {idx[0]}, element "
                             f"{flat} (block {flat >> 2}, lane {flat & 3}), got {float(got16[tuple(idx)])!r}, model "
                             f"{scale * float(z_model[tuple(idx)])!r}")


@pytest.mark.parametrize("shape", [(2, 3, 4, 4), (2, 3, 3, 5), (2, 4, 32, 32)], ids=["hw16", "hw15", "hw1024"])
def test_randn_against_the_model(shape):
    """``sp_randn_f16``: both purposes, scale 1 and the initial sigma, aligned and 2 bytes off; a video's values do not depend
    on what it is batched with."""
    from vdpp_amd.hip import ops
    nb, f, h, w = shape
    seeds = (42, 2 ** 63 - 1)
    for step, purpose, scale in ((0, nm.INITIAL, 1.0), (0, nm.INITIAL, 700.0007), (5, nm.STEP, 1.0)):
        z = np.stack([nm.video_normals(s, f, h, w, step, purpose) for s in seeds])
        out = torch.full((nb, 4, f, h, w), float("nan"), dtype=torch.float16, device=DEV)
        ops.randn(out, _seeds(seeds), scale=scale, step=step, purpose=purpose)
        got = out.cpu().numpy()
        _check_z(got, z, np.float32(scale), f"step {step} purpose {purpose} scale {scale}")
        off = _off_by_one_f16(torch.full_like(out, float("nan")))
        ops.randn(off, _seeds(seeds), scale=scale, step=step, purpose=purpose)
        assert np.array_equal(off.cpu().numpy().view(np.uint16), got.view(np.uint16)), "2 bytes off: other values"
        for b in range(nb):
            alone = torch.empty((1, 4, f, h, w), dtype=torch.float16, device=DEV)
            ops.randn(alone, _seeds(seeds[b:b + 1]), scale=scale, step=step, purpose=purpose)
            assert np.array_equal(alone.cpu().numpy()[0].view(np.uint16), got[b].view(np.uint16)), f"video {b} alone"
    a, b = got[0], got[1]
    assert not np.array_equal(a, b), "two seeds, the same values"


@pytest.mark.parametrize("shape", nm.SHAPES, ids=["hw16", "hw15", "windows-hw16", "windows-hw15"])
def test_z_recovered_from_the_tails(shape):
    """``x = 0``, ``eps = 0``, ``n = 1``: both tails return fp16(z) (for 2M beside ``D = 0``), in both kernels, both 2M forms
    and both pixel forms, bit for bit the same value for the same element; other steps and other seeds give other values."""
    nb, ft, window, stride, h, w = shape
    n_win = (ft - window) // stride + 1
    eps = np.zeros((n_win * nb * window * h * w, 8), dtype=np.float16)
    steps = nm.kernel_steps()
    seen = {}
    for name, st in steps.items():
        z = nm.step_noise(nm.SEEDS, shape, st["step"])
        for channels in (4, 8):
            state = np.zeros((nb, channels, ft, h, w), dtype=np.float16)
            forms = [False] + ([True] if (h * w) % 4 == 0 else [])
            outs = [_run(state, eps, None, None, 0, shape, st, _seeds(nm.SEEDS), misalign=m, n=1.0) for m in forms]
            _check_z(outs[0][:, :4], z, np.float32(1.0), f"{name}, {channels} channels")
            if channels == 8:
                assert not outs[0][:, 4:].any(), "D carries noise"
            for o in outs[1:]:
                assert np.array_equal(o.view(np.uint16), outs[0].view(np.uint16)), f"{name}: one pixel per thread gives other values"
            seen[(name, channels)] = outs[0][:, :4]
    assert np.array_equal(seen[("history", 4)], seen[("history", 8)]), "Euler ancestral and 2M SDE draw other noise"
    assert not np.array_equal(seen[("history", 4)], seen[("first-order", 4)]), "two steps, the same noise"
    assert not np.array_equal(seen[("history", 4)][0], seen[("history", 4)][1]), "two seeds, the same noise"


# ------------------------------------------------------------------------------------------------ the steps
def _within(got, want, terms, nz, shape, what):
    err, lim = np.abs(got.astype(np.float64) - want), nm.bound(want, terms, nz, shape)
    ok = err <= lim
    print(f"{what}: worst ratio to the bound {np.nanmax(err / lim):.3f}")
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} outside the bound, worst ratio {np.nanmax(err / lim):.3f}"


@pytest.mark.parametrize("shape", nm.SHAPES, ids=["hw16", "hw15", "windows-hw16", "windows-hw15"])
@pytest.mark.parametrize("guidance", GUIDANCE)
def test_steps_against_the_fp64_model(guidance, shape):
    """Both tails at a second-order step and at step 0 (``c2 == 0``: NaN in the history channels is not read), without
    guidance, with one ``[F]`` row and with ``[B][F]`` rows, out of place, in place and (``H*W % 4 == 0``) from a view 2 bytes
    off, which takes one pixel per thread."""
    seeds = _seeds(nm.SEEDS)
    for name, st in nm.kernel_steps().items():
        state, ec, eu, g, ld_g = _case(shape, guidance, 8, name, st)
        want_x, want_d, terms, d_terms, nz = nm.dpmpp2m_sde_step(state, ec, eu, g, nm.SEEDS, st["step"], shape=shape,
                                                                 sigma=st["sigma"], **st["sde"])
        lat, ec4, eu4, g4, ld_g4 = _case(shape, guidance, 4, name, st)
        want_e, terms_e, nz_e = nm.euler_ancestral_step(lat, ec4, eu4, g4, nm.SEEDS, st["step"], shape=shape, sigma=st["sigma"],
                                                        **st["euler"])
        for form in ("out of place", "in place") + (("2 bytes off",) if (shape[4] * shape[5]) % 4 == 0 else ()):
            kw = dict(in_place=form == "in place", misalign=form == "2 bytes off")
            got = _run(state, ec, eu, g, ld_g, shape, st, seeds, **kw)
            assert np.isfinite(got).all(), f"{name}, {form}: a NaN was read"
            _within(got[:, :4], want_x, terms, nz, shape, f"2M SDE {name} x' ({form})")
            _within(got[:, 4:], want_d, d_terms, 0.0, shape, f"2M SDE {name} D ({form})")
            got = _run(lat, ec4, eu4, g4, ld_g4, shape, st, seeds, **kw)
            _within(got, want_e, terms_e, nz_e, shape, f"Euler ancestral {name} ({form})")


@pytest.mark.parametrize("guidance", GUIDANCE)
def test_bit_for_bit_relations_of_the_tails(guidance):
    """On real inputs: the four-pixel and the one-pixel form (Euler ancestral); video b of a batch of two against the video alone with its seed;
    one window with its weight table against the unwindowed call; ``n == 0`` against the deterministic entry points."""
    from tests.golden import make_sampler_tail_golden as golden
    seeds = _seeds(nm.SEEDS)
    for shape in (nm.SHAPES[0], nm.SHAPES[2]):
        nb, ft, window, stride, h, w = shape
        n_win = (ft - window) // stride + 1
        for name, st in nm.kernel_steps().items():
            for channels in (4, 8):
                state, ec, eu, g, ld_g = _case(shape, guidance, channels, name, st)
                what = f"{shape}, {name}, {channels} channels"
                got = _run(state, ec, eu, g, ld_g, shape, st, seeds)
                assert np.isfinite(got).all()
                if channels == 4:
                    # (2M stores x' and D "as today": a scalar store rounds the last fma once, a packed one twice, so its two
                    # forms agree bit for bit where that fma is exact -- test_z_recovered_from_the_tails -- and within the
                    # bound elsewhere -- test_steps_against_the_fp64_model, "2 bytes off")
                    narrow = _run(state, ec, eu, g, ld_g, shape, st, seeds, misalign=True)
                    assert np.array_equal(narrow.view(np.uint16), got.view(np.uint16)), f"{what}: pixel forms differ"
                rows = lambda t, b: None if t is None else \
                    np.ascontiguousarray(t.reshape(n_win, nb, -1, t.shape[1])[:, b:b + 1]).reshape(-1, t.shape[1])
                for b in range(nb):
                    gb = g if g is None or g.ndim == 1 else g[b:b + 1]
                    alone = _run(state[b:b + 1], rows(ec, b), rows(eu, b), gb, ld_g, (1,) + shape[1:], st, seeds[b:b + 1].clone())
                    assert np.array_equal(alone[0].view(np.uint16), got[b].view(np.uint16)), f"{what}: video {b} alone differs"
                if window == ft:
                    table = _run(state, ec, eu, g, ld_g, shape, st, seeds, one_window_table=True)
                    assert np.array_equal(table.view(np.uint16), got.view(np.uint16)), f"{what}: one window differs"
                # n == 0: the deterministic kernels' bytes, seeds not read
                det = dict(sigma=st["sigma"], sigma_next=st["euler"]["sigma_down"], **{k: st["sde"][k] for k in ("a", "b", "c1", "c2")})
                want = golden.run_tail(state, ec, eu, g, ld_g, shape, det, rows_kernel=window == ft)
                quiet = _run(state, ec, eu, g, ld_g, shape, st, None, n=0.0)
                assert np.array_equal(quiet.view(np.uint16), want.view(np.uint16)), f"{what}: n == 0 is not the deterministic tail"
                assert not np.array_equal(quiet[:, :4], got[:, :4])


# ------------------------------------------------------------------------------------------------ the whole step
def _build(c=64, seed=3):
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict
    cfg = UNetConfig.tiny(c)
    sd = random_state_dict(cfg, seed=seed, dtype=torch.float16)
    return cfg, sd, SVDUNetHIP(cfg, sd, DEV)


def _model(hip, sampler, steps=N_STEPS, **kw):
    from vdpp_amd.models.svd_unet import StableVideoUNet
    return StableVideoUNet(unet=hip, timesteps=StableVideoUNet._default_timestep_schedule(steps), sampler=sampler, **kw)


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


PAIRS = [("euler_a", "euler"), ("dpmpp_2m_sde", "dpmpp_2m")]


@pytest.mark.parametrize("sampler,plain", PAIRS)
def test_eta_zero_is_the_deterministic_sampler_bit_for_bit(sampler, plain):
    """Whole steps of the tiny model: ``eta = 0`` gives ``n = 0`` and the deterministic sampler's constants, so the stored-eps
    route and the tail without noise return the bytes of ``sampler="euler"`` (its tail fused into ``conv_out``) and
    ``"dpmpp_2m"``; unwindowed and with windows.  With ``eta = 1`` the same call gives another sample."""
    cfg, sd, hip = _build(seed=23)
    frames, h, w = 4, 8, 16
    g, emb, img = _conditioning(cfg, frames, h, w, nb=2)
    for stride, ft in ((None, frames), (2, 8)):
        quiet, loud, ref = (_model(hip, sampler, eta=0.0, window_stride=stride), _model(hip, sampler, window_stride=stride),
                            _model(hip, plain, window_stride=stride))
        assert quiet.stochastic and quiet.state_channels == ref.state_channels
        for guidance in (None, [3.0, 1.5]):
            kw = dict(guidance_scale=guidance, num_frames=frames)
            seeded = quiet.prepare_conditioning(emb, img, noise_seed=[5, 6], **kw)
            for step in (0, 7, N_STEPS - 1):
                state = _state(ref, g, 2, ft, h, w)
                want = ref(state, step, conditioning=ref.prepare_conditioning(emb, img, **kw))
                assert torch.equal(quiet(state, step, conditioning=seeded), want), f"stride {stride}, guidance {guidance}, step {step}"
                if step < N_STEPS - 1:
                    assert not torch.equal(loud(state, step, conditioning=seeded)[:, :4], want[:, :4])


@pytest.mark.parametrize("sampler,plain", PAIRS)
def test_model_step_is_the_tail_behind_the_models_eps(sampler, plain):
    """``forward`` against ``noise_model`` on the eps rows the same engine stores, guided, for two videos with their own seeds;
    a conditioning without seeds is refused with a text that names ``noise_seed=``; one window equals the unwindowed model."""
    cfg, sd, hip = _build(seed=5)
    model, windowed = _model(hip, sampler), _model(hip, sampler, window_stride=2)
    frames, h, w, step = 3, 8, 16, 12
    g, emb, img = _conditioning(cfg, frames, h, w, nb=2)
    seeds = [11, 2 ** 62 + 3]
    cond = model.prepare_conditioning(emb, img, guidance_scale=[3.0, 1.5], num_frames=frames, noise_seed=seeds)
    assert cond.noise_seeds.dtype == torch.int64 and cond.noise_seeds.tolist() == seeds
    state = _state(model, g, 2, frames, h, w)
    got = model(state, step, conditioning=cond)
    assert torch.equal(windowed(state, step, conditioning=cond), got), "one window differs from the unwindowed model"
    sigma = model._sigma_host[step]
    x = model.sample_of(state).contiguous()
    eps_c, eps_u = model._unet_passes(x, cond, step, 1.0 / (sigma * sigma + 1.0) ** 0.5)
    shape = (2, frames, frames, frames, h, w)
    args = (state.cpu().numpy(), eps_c.cpu().numpy(), eps_u.cpu().numpy(), cond.guidance32.cpu().numpy(), seeds, step)
    if sampler == "euler_a":
        down, n = model._noise_coef[step]
        want, terms, nz = nm.euler_ancestral_step(*args, shape=shape, sigma=sigma, sigma_down=down, n=n)
    else:
        a, b, c1, c2, n = model._noise_coef[step]
        want, want_d, terms, d_terms, nz = nm.dpmpp2m_sde_step(*args, shape=shape, sigma=sigma, a=a, b=b, c1=c1, c2=c2, n=n)
        _within(got[:, 4:].cpu().numpy(), want_d, d_terms, 0.0, shape, f"{sampler} D")
    assert n > 0
    _within(got[:, :4].cpu().numpy(), want, terms, nz, shape, f"{sampler} x'")
    with pytest.raises(ValueError, match="noise_seed="):
        model(state, step, conditioning=model.prepare_conditioning(emb, img, guidance_scale=[3.0, 1.5], num_frames=frames))
    with pytest.raises(ValueError, match=r"\[0, 2\^63\)"):
        cond.with_noise_seed(-1)
    other = cond.with_noise_seed([11, 12])
    assert other.image_latents is cond.image_latents and other.noise_seeds.tolist() == [11, 12]
    moved = model(state, step, conditioning=other)
    assert torch.equal(moved[0], got[0]) and not torch.equal(moved[1, :4], got[1, :4]), "a video's noise follows its own seed"


@pytest.mark.parametrize("sampler,plain", PAIRS)
def test_batched_cfg_and_windows(sampler, plain):
    """Three windows, guided: ``batched_cfg`` against sequential CFG to the 1e-3 the deterministic window path is held to (the
    noise is the same function of seed, step and element in both)."""
    cfg, sd, hip = _build(seed=17)
    seq, bat = _model(hip, sampler, window_stride=2), _model(hip, sampler, window_stride=2, batched_cfg=True)
    window, ft, h, w = 4, 8, 8, 16
    g, emb, img = _conditioning(cfg, window, h, w, seed=5)
    for m in (seq, bat):
        m.set_conditioning(emb, img, guidance_scale=3.0, num_frames=window, noise_seed=77)
    state = _state(seq, g, 1, ft, h, w)
    a, b = seq(state, 7), bat(state, 7)
    assert a.shape == state.shape and torch.isfinite(a).all() and torch.isfinite(b).all()
    assert rel_l2(b[:, :4].float(), a[:, :4].float()) <= 1e-3


@pytest.mark.parametrize("sampler,plain", PAIRS)
def test_graph_replay_equals_eager_and_reads_the_current_seeds(sampler, plain):
    """The first call captures, the later ones replay with other data, and then with other SEEDS in the lane's conditioning
    copy: the replay reads the seeds of the lane's current request, not those it was captured with."""
    cfg, sd, hip = _build(seed=19)
    eager, graphed = _model(hip, sampler), _model(hip, sampler)
    graphed.enable_graphs()
    frames, h, w = 3, 8, 16
    g, emb, img = _conditioning(cfg, frames, h, w)
    kw = dict(guidance_scale=2.5, num_frames=frames)
    outs = []
    for seed in (3, 3, 2 ** 63 - 1):
        cond = eager.prepare_conditioning(emb, img, noise_seed=seed, **kw)
        for step in (0, 7):
            state = _state(eager, g, 1, frames, h, w)
            want = eager(state, step, conditioning=cond)
            assert torch.equal(graphed(state, step, conditioning=cond), want), f"seed {seed} step {step}"
        outs.append((state, want))
    state, want = outs[1]
    other = eager(state, 7, conditioning=eager.prepare_conditioning(emb, img, noise_seed=4, **kw))
    assert not torch.equal(other[:, :4], want[:, :4]), "two seeds, the same sample"
    graphed.enable_graphs(False)
    # the model's own conditioning (set_conditioning) replays too
    own = _model(hip, sampler)
    own.enable_graphs()
    for m in (eager, own):
        m.set_conditioning(emb, img, noise_seed=9, **kw)
    for trial in range(2):
        state = _state(eager, g, 1, frames, h, w)
        assert torch.equal(own(state, 7), eager(state, 7)), f"own conditioning, trial {trial}"
    own.enable_graphs(False)


@pytest.mark.parametrize("sampler,plain", PAIRS)
def test_state_handed_between_two_models_after_every_step(sampler, plain):
    """Steps 0..5 in one model == steps 0..k there and k+1..5 in a second model that is handed nothing but the tensor (and
    the request's conditioning with its seed): no generator state lives anywhere.  The latent starts from the device noise."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, hip = _build(seed=23)
    first, second = _model(hip, sampler, steps=6), _model(SVDUNetHIP(cfg, sd, DEV), sampler, steps=6)
    frames, h, w = 3, 8, 16
    g, emb, img = _conditioning(cfg, frames, h, w)
    for m in (first, second):
        m.set_conditioning(emb, img, guidance_scale=2.0, num_frames=frames, noise_seed=1234)
    noise = first.initial_noise(1234, frames, h, w)
    z = nm.video_normals(1234, frames, h, w, 0, nm.INITIAL)[None]
    _check_z(noise.cpu().numpy(), z, np.float32(first.init_noise_sigma), "initial_noise")
    states = [first.init_state(noise)]
    for step in range(6):
        states.append(first(states[-1], step))
    assert torch.isfinite(states[-1]).all()
    for k in range(5):
        state = states[k + 1].clone()
        for step in range(k + 1, 6):
            state = second(state, step)
        assert torch.equal(state, states[-1]), f"hand-over after step {k}"


# ------------------------------------------------------------------------------------------------ end to end
def _generate_args(src, out, rendezvous, seed):
    return ["--backend", "gloo", "--init-method", f"file://{rendezvous}", "--log-level", "WARNING", "--random-init", "--tiny",
            "--input-image", str(src), "--height", "64", "--width", "128", "--num-frames", "3", "--sampler", "dpmpp_2m_sde",
            "--noise", "device", "--seed", str(seed), "--total-steps", "6", "--output", str(out)]


def test_generate_mode_on_one_and_on_two_ranks(monkeypatch, tmp_path):
    """``modes.generate --sampler dpmpp_2m_sde --noise device --seed 7`` in this process and as two rank processes that share
    the GPU (a boundary after step 2): the same frames byte for byte; ``--seed 8`` writes other frames."""
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.modes import generate
    rng = np.random.default_rng(5)
    src = tmp_path / "in.png"
    Image.fromarray(rng.integers(0, 256, (96, 160, 3), dtype=np.uint8)).save(src)
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    generate.main(_generate_args(src, tmp_path / "one.npy", tmp_path / "rendezvous_one", 7))
    generate.main(_generate_args(src, tmp_path / "other.npy", tmp_path / "rendezvous_other", 8))
    assert not torch.distributed.is_initialized()
    one, other = np.load(tmp_path / "one.npy"), np.load(tmp_path / "other.npy")
    assert one.shape == (3, 64, 128, 3) and one.dtype == np.uint8 and int(one.max()) > int(one.min())
    assert other.tobytes() != one.tobytes(), "another seed wrote the same frames"
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, "-m", "vdpp_amd.modes.generate"]
                                      + _generate_args(src, tmp_path / "two.npy", tmp_path / "rendezvous_two", 7),
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(log[-3000:] for log in logs)
    two = np.load(tmp_path / "two.npy")
    assert two.tobytes() == one.tobytes(), "two ranks gave other frames than one"
