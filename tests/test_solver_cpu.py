"""DPM-Solver++(2M) without a GPU: the host coefficients (``models/solver_schedule.py``), the fp64 statement of the update
(``tests/solver_model.py``) against the pinned Euler oracle, the solver's order on an analytic denoiser, and the 8-channel
state (sample ++ previous denoised estimate) through the step pipeline over Gloo."""

import logging
import math
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import solver_model as sm
from vdpp_amd.models.euler_schedule import karras_sigma_table
from vdpp_amd.models.solver_schedule import dpmpp_2m_coefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVERGENCE = os.path.join(ROOT, "profiles", "sampler_convergence.txt")


def _sigmas(n):
    return karras_sigma_table(n).double().tolist()


# ------------------------------------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("n", [2, 6, 25, 40])
def test_coefficient_identities(n):
    sig = _sigmas(n)
    co = dpmpp_2m_coefficients(sig)
    assert len(co) == n
    for i, (a, b, c1, c2) in enumerate(co):
        assert a == sig[i + 1] / sig[i] and 0.0 <= a < 1.0
        assert abs(a + b - 1.0) <= 1e-15 and abs(c1 - c2 - 1.0) <= 1e-15 and c2 >= 0.0
    assert co[0][2:] == (1.0, 0.0) and co[-1][2:] == (1.0, 0.0), "the first and the last step are first order"
    assert co[-1][:2] == (0.0, 1.0), "sigma' = 0: x' = D"
    assert all(c2 > 0.0 for _, _, _, c2 in co[1:-1])
    # a torch table (what StableVideoUNet holds) and a list give the same numbers
    assert dpmpp_2m_coefficients(karras_sigma_table(n)) == dpmpp_2m_coefficients(karras_sigma_table(n).tolist())


def test_geometric_sigmas_give_c2_of_one_half():
    sig = [2.0 ** (5 - k) for k in range(9)]
    co = dpmpp_2m_coefficients(sig)
    assert co[0][3] == 0.0 and all(c2 == 0.5 and c1 == 1.5 for _, _, c1, c2 in co[1:])
    co = dpmpp_2m_coefficients(sig + [0.0])
    assert co[-1][2:] == (1.0, 0.0) and all(c2 == 0.5 for _, _, _, c2 in co[1:-1])


def test_coefficients_refuse_a_table_that_does_not_decrease():
    for bad in ([1.0], [1.0, 1.0], [1.0, 2.0], [0.0, 0.0], [2.0, 1.0, 0.0, 0.0], [-1.0, -2.0]):
        with pytest.raises(ValueError):
            dpmpp_2m_coefficients(bad)


@pytest.mark.parametrize("n", [6, 25, 80])
def test_coefficients_agree_with_k_diffusion(n):
    """k-diffusion's ``sample_dpmpp_2m``, written out as it stands there (t = -log sigma, expm1), applied to random scalars:
    the same x' from (x, D, D_prev) to 1e-12."""
    sig = _sigmas(n)
    co = dpmpp_2m_coefficients(sig)
    rng = np.random.default_rng(n)
    t_fn = lambda s: -math.log(s)                                 # noqa: E731
    for i in range(n):
        x, den, old = rng.standard_normal(3)
        if sig[i + 1] == 0.0:
            want = den                       # (k-diffusion: sigma_fn(t_next)/sigma_fn(t) = 0 and -expm1(-inf) = 1)
        else:
            t, t_next = t_fn(sig[i]), t_fn(sig[i + 1])
            h = t_next - t
            if i == 0:
                want = (sig[i + 1] / sig[i]) * x - math.expm1(-h) * den
            else:
                h_last = t - t_fn(sig[i - 1])
                r = h_last / h
                den_d = (1 + 1 / (2 * r)) * den - (1 / (2 * r)) * old
                want = (sig[i + 1] / sig[i]) * x - math.expm1(-h) * den_d
        a, b, c1, c2 = co[i]
        got = a * x + b * (c1 * den - c2 * old)
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), f"step {i}"


# ------------------------------------------------------------------------------------------------ Euler identity
class _StubUNet:
    """A UNet-shaped callable for ``svd_step``: eps from the input sample and the conditioning, on a grid of quarters so
    that the fp16 guidance mix of the model and the fp32 one of ``svd_step`` are both exact."""

    def __call__(self, sample, timestep, encoder_hidden_states, added_time_ids, return_dict=False):
        x = sample[:, :, :4].float()
        shift = float(encoder_hidden_states.float().abs().sum() > 0)
        eps = torch.round(4.0 * torch.sin(3.0 * x + shift + float(timestep))) / 4.0
        return (eps,)


@pytest.mark.parametrize("guidance", [None, 3.0])
def test_first_order_update_is_the_oracles_euler_step(guidance):
    from oracle.svd_step_ref import svd_step
    from vdpp_amd.models.euler_schedule import continuous_timesteps

    n = 25
    sig32 = karras_sigma_table(n)
    sig, co = sig32.double().tolist(), dpmpp_2m_coefficients(sig32)
    b, f, h, w = 2, 5, 3, 4
    g = torch.Generator().manual_seed(3)
    emb, img = torch.randn(b, 1, 8, generator=g), torch.randn(b, 4, f, h, w, generator=g)
    ids = torch.tensor([[5.0, 127.0, 0.02]])
    stub = _StubUNet()
    for step in (0, 1, 12, 23, 24):
        x = (torch.randn(b, 4, f, h, w, generator=g) * (sig[step] + 1)).half().float()
        with torch.no_grad():
            want = svd_step(stub, x, step, sigmas=sig32, timesteps=continuous_timesteps(sig32), image_embeddings=emb,
                            image_latents=img, added_time_ids=ids, guidance_scale=guidance, dtype=torch.float32)
        # the same eps rows the oracle's passes produced, through the model's own guidance mix
        scaled = x / ((sig32[step] ** 2 + 1) ** 0.5)
        t = continuous_timesteps(sig32)[step]

        def rows(im, em):
            s = torch.cat([scaled, im], dim=1).permute(0, 2, 1, 3, 4)
            return stub(s, t, em, ids)[0].permute(0, 1, 3, 4, 2).reshape(-1, 4).numpy()

        eps_c = rows(img, emb)
        eps_u = rows(torch.zeros_like(img), torch.zeros_like(emb)) if guidance else None
        gs = torch.linspace(1.0, guidance, f).numpy() if guidance else None
        state = np.concatenate([x.numpy(), np.full((b, 4, f, h, w), np.nan, np.float32)], axis=1)
        a, bb, _, _ = co[step]
        got, den, _ = sm.dpmpp2m_step(state, eps_c, eps_u, gs, sigma=sig[step], a=a, b=bb, c1=1.0, c2=0.0)
        assert np.isfinite(got).all(), "c2 = 0 must not read the history channels"
        err = np.linalg.norm(got - want.double().numpy()) / np.linalg.norm(want.double().numpy())
        assert err <= 1e-6, f"step {step}: rel_l2={err:.3e}"
        if step == n - 1:
            assert np.array_equal(got, den), "sigma' = 0: x' = D"
        # and the model's own fp64 Euler statement
        e = sm.rows_to_planes(eps_c, b, f, h, w) if not guidance else sm.guidance_mix_f16(
            sm.rows_to_planes(eps_c, b, f, h, w), sm.rows_to_planes(eps_u, b, f, h, w), gs.reshape(1, 1, f, 1, 1))
        eul = sm.euler_step(x.numpy(), e.astype(np.float64), sig[step], sig[step + 1])
        assert np.linalg.norm(got - eul) <= 1e-12 * np.linalg.norm(eul)


# ------------------------------------------------------------------------------------------------ order of the solver
def _analytic_error(n, s, second_order):
    """Relative error at sigma = 0 on ``karras_sigma_table(n)`` with the denoiser D(x, sigma) = x*s^2/(s^2 + sigma^2), whose
    probability-flow solution is x(0) = x(sigma_0)*s/sqrt(s^2 + sigma_0^2)."""
    sig = _sigmas(n)
    co = dpmpp_2m_coefficients(sig)
    x, old = 1.0, 0.0
    for i in range(n):
        den = x * s * s / (s * s + sig[i] ** 2)
        a, b, c1, c2 = co[i]
        if not second_order:
            c1, c2 = 1.0, 0.0
        x, old = a * x + b * (c1 * den - c2 * old), den
    exact = s / math.sqrt(s * s + sig[0] ** 2)
    return abs(x - exact) / exact


def _convergence_text():
    lines = ["Relative error at sigma = 0 of the two samplers on models/euler_schedule.karras_sigma_table(N) (sigma 700 -> 0.002,",
             "rho 7) with the analytic denoiser D(x, sigma) = x*s^2/(s^2 + sigma^2), exact solution x(0) = x(sigma_0)*s/sqrt(s^2 +",
             "sigma_0^2); fp64, on the CPU.  Written by tests/test_solver_cpu.py with SAMPLER_WRITE_CONVERGENCE=1; the test fails",
             "when it is stale.  Not a statement about image quality on trained weights.",
             "Taken on top of commit 8fd490f, on the CPU (host arithmetic only; no GPU is involved).", "",
             f"{'s':>5}{'N':>5}{'euler(N)':>12}{'euler(2N)':>12}{'dpmpp_2m(N)':>13}{'2m(N)<eul(2N)':>15}"]
    for s in (0.5, 1.0, 4.0):
        for n in (10, 16, 20, 25, 40, 80):
            e1, e2, m = _analytic_error(n, s, False), _analytic_error(2 * n, s, False), _analytic_error(n, s, True)
            lines.append(f"{s:>5.1f}{n:>5d}{e1:>12.3e}{e2:>12.3e}{m:>13.3e}{str(m < e2):>15}")
    lines.append("")
    for s in (0.5, 1.0, 4.0):
        lines.append(f"s = {s:.1f}: err(40)/err(80) = {_analytic_error(40, s, True) / _analytic_error(80, s, True):.2f} (dpmpp_2m), "
                     f"{_analytic_error(40, s, False) / _analytic_error(80, s, False):.2f} (euler)")
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("s", [0.5, 1.0, 4.0])
def test_second_order_on_an_analytic_denoiser(s):
    for n in (25, 40):
        m, e2 = _analytic_error(n, s, True), _analytic_error(2 * n, s, False)
        assert m < e2, f"s={s}: dpmpp_2m at {n} steps ({m:.3e}) is not more accurate than Euler at {2 * n} ({e2:.3e})"
    assert _analytic_error(40, s, True) / _analytic_error(80, s, True) >= 3.5
    assert _analytic_error(40, s, False) / _analytic_error(80, s, False) <= 2.2


def test_convergence_table_is_current():
    text = _convergence_text()
    if os.environ.get("SAMPLER_WRITE_CONVERGENCE") == "1":
        with open(CONVERGENCE, "w") as fh:
            fh.write(text)
    with open(CONVERGENCE) as fh:
        assert fh.read() == text, "profiles/sampler_convergence.txt is stale: run this test with SAMPLER_WRITE_CONVERGENCE=1"


# ------------------------------------------------------------------------------------------------ state through the pipeline
class _Analytic2M(torch.nn.Module):
    """The 8-channel protocol of ``StableVideoUNet(sampler="dpmpp_2m")`` on the CPU: stateless, the history in channels 4-7,
    the package's coefficients, the analytic denoiser (with a per-channel s, so that the planes differ)."""

    def __init__(self, n):
        super().__init__()
        self.sig = _sigmas(n)
        self.coef = dpmpp_2m_coefficients(self.sig)
        self.register_buffer("s2", torch.tensor([0.25, 1.0, 4.0, 16.0], dtype=torch.float64).view(1, 4, 1, 1, 1))

    def init_state(self, noise):
        return torch.cat([noise, torch.zeros_like(noise)], dim=1)

    def forward(self, state, step):
        x, old = state[:, :4], state[:, 4:]
        a, b, c1, c2 = self.coef[step]
        den = x * (self.s2 / (self.s2 + self.sig[step] ** 2))
        dd = den if c2 == 0.0 else c1 * den - c2 * old
        return torch.cat([a * x + b * dd, den], dim=1)


def _noise(i):
    return torch.randn(1, 4, 2, 3, 5, generator=torch.Generator().manual_seed(50 + i), dtype=torch.float64) * 700.0


def _plain_loop(n, i, drop_history=False):
    model = _Analytic2M(n)
    state = model.init_state(_noise(i))
    for step in range(n):
        if drop_history:
            state[:, 4:] = 0.0
        state = model(state, step)
    return state


def _run_pipeline(rank, ws, n, mode, samples, init_file, out_file):
    from vdpp_amd.distributed import finalize_distributed, init_distributed
    from vdpp_amd.pipeline import LatentSpec, PipelineConfig, PipelineStage, run_pipeline_latents

    torch.set_num_threads(1)
    if ws > 1:
        init_distributed(backend="gloo", rank=rank, world_size=ws, init_method=f"file://{init_file}")
    model = _Analytic2M(n)
    spec = LatentSpec(shape=torch.Size((1, 8, 2, 3, 5)), dtype=torch.float64, device=torch.device("cpu"))
    quiet = logging.getLogger("quiet"); quiet.setLevel(logging.ERROR)
    supplier = (lambda i: model.init_state(_noise(i))) if rank == 0 else None
    ts = list(range(n))                                   # a multistep solver walks the sigma table in index order
    with torch.no_grad():
        if mode == "rotate":
            stage = PipelineStage(model, PipelineConfig(total_steps=n, world_size=ws, rank=rank, timesteps=ts, latent_spec=spec,
                                                        balanced=True, rotate=True), logger=quiet)
            outs = stage.run_many(samples, input_supplier=supplier)
            stage.drain()
        else:
            outs = run_pipeline_latents(model, total_steps=n, timesteps=ts, world_size=ws, rank=rank, latent_spec=spec,
                                        num_samples=samples, input_supplier=supplier, logger=quiet,
                                        balanced=mode == "balanced")
    if rank == ws - 1:
        torch.save(outs, out_file)
    else:
        assert outs is None
    if ws > 1:
        finalize_distributed()


@pytest.mark.parametrize("ws,n,mode", [(1, 6, "chain"), (2, 6, "chain"), (3, 6, "chain"), (1, 7, "balanced"), (2, 7, "balanced"),
                                       (3, 7, "balanced"), (2, 7, "rotate"), (3, 7, "rotate")])
def test_solver_history_survives_stage_boundaries(ws, n, mode):
    """Stage boundaries fall between different pairs of steps at every world size and, with the rotating split, from sample to
    sample: the finished 8-channel states are bit-identical to the plain loop, which they could not be had a boundary lost the
    history (dropping it changes the result)."""
    samples = 4
    with tempfile.TemporaryDirectory() as td:
        out_file = os.path.join(td, "out.pt")
        if ws == 1:
            _run_pipeline(0, 1, n, mode, samples, None, out_file)
        else:
            mp.spawn(_run_pipeline, args=(ws, n, mode, samples, os.path.join(td, "init"), out_file), nprocs=ws, join=True)
        outs = torch.load(out_file)
    assert len(outs) == samples
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for i, got in enumerate(outs):
            want = _plain_loop(n, i)
            assert got.shape == (1, 8, 2, 3, 5) and torch.equal(got, want), f"sample {i}"
            assert not torch.equal(want[:, :4], _plain_loop(n, i, drop_history=True)[:, :4])
    finally:
        torch.set_num_threads(threads)
