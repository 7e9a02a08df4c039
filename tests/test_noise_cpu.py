"""The stochastic samplers on the CPU: the generator's known answers and moments (``tests/noise_model.py``), the host
coefficients of Euler ancestral and DPM-Solver++(2M) SDE (``models/solver_schedule.py``), the planted mistakes the GPU test's
bound must see, and the closed-form variance table ``profiles/sde_convergence.txt``."""

import math
import os

import numpy as np
import pytest

from tests import noise_model as nm
from tests import window_model as wm
from vdpp_amd.models.euler_schedule import karras_sigma_table
from vdpp_amd.models.solver_schedule import (SAMPLERS, dpmpp_2m_coefficients, dpmpp_2m_sde_coefficients,
                                              euler_ancestral_coefficients)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVERGENCE = os.path.join(ROOT, "profiles", "sde_convergence.txt")


def _sigmas(n):
    return karras_sigma_table(n).double().tolist()


# ------------------------------------------------------------------------------------------------ the generator
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = nm.philox4x32_10(*counter, *key)
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_blocks_follow_the_address():
    """``blocks`` is Philox of counter (j, step, purpose, 0) under the key (seed low, seed high)."""
    seed = 2 ** 63 - 1
    got = nm.blocks(seed, [0, 5, 2 ** 32 - 1], step=3, purpose=1)
    for row, j in zip(got, (0, 5, 2 ** 32 - 1)):
        want = nm.philox4x32_10(j, 3, 1, 0, seed & 0xFFFFFFFF, seed >> 32)
        assert [int(v) for v in row] == [int(v) for v in want]
    assert not np.array_equal(nm.blocks(seed, [0], 3, 1), nm.blocks(seed, [0], 3, 0))
    assert not np.array_equal(nm.blocks(seed, [0], 3, 1), nm.blocks(seed, [0], 4, 1))
    assert not np.array_equal(nm.blocks(seed, [0], 3, 1), nm.blocks(seed - 1, [0], 3, 1))


def test_uniform_is_exact_in_fp32_and_inside_the_unit_interval():
    a = np.array([0, 511, 512, 2 ** 32 - 1], dtype=np.uint64)
    u = nm.uniform(a)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24


def test_normals_have_the_moments_of_a_standard_normal():
    """2^22 values of seed 42: mean, variance and fourth moment within five standard errors of 0, 1 and 3."""
    n = 2 ** 22
    z = nm.normals_of_words(nm.blocks(42, np.arange(n // 4), step=0, purpose=nm.INITIAL)).ravel()
    assert z.size == n and np.isfinite(z).all()
    mean, var, m4 = z.mean(), z.var(), (z ** 4).mean()
    print(f"|mean| {abs(mean):.2e} (limit {5 / math.sqrt(n):.2e}), |var-1| {abs(var - 1):.2e} (limit {5 * math.sqrt(2 / n):.2e}), "
          f"|m4-3| {abs(m4 - 3):.2e} (limit {5 * math.sqrt(96 / n):.2e})")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(m4 - 3) <= 5 * math.sqrt(96 / n)


def test_element_normals_are_the_lanes_of_the_blocks():
    z = nm.video_normals(7, 3, 3, 5, step=2, purpose=nm.STEP)
    z4 = nm.normals_of_words(nm.blocks(7, np.arange(4 * 3 * 15 // 4), 2, nm.STEP))
    assert np.array_equal(z.ravel(), z4.ravel())


# ------------------------------------------------------------------------------------------------ coefficients
def test_sampler_names():
    assert SAMPLERS[:2] == ("euler", "dpmpp_2m") and set(SAMPLERS[2:]) == {"euler_a", "dpmpp_2m_sde"}


@pytest.mark.parametrize("n", [2, 6, 25, 40])
def test_euler_ancestral_coefficient_identities(n):
    sig = _sigmas(n)
    assert euler_ancestral_coefficients(sig, 0.0, 1.0) == [(s, 0.0) for s in sig[1:]], "eta = 0 is the Euler sampler, exactly"
    for eta, s_noise in ((1.0, 1.0), (0.5, 1.0), (1.0, 0.7), (3.0, 1.0)):
        co = euler_ancestral_coefficients(sig, eta, s_noise)
        assert len(co) == n and co[-1] == (0.0, 0.0)
        for i, (down, noise) in enumerate(co[:-1]):
            s, s_next = sig[i], sig[i + 1]
            up = noise / s_noise
            assert 0.0 <= down <= s_next and 0.0 <= up <= s_next
            assert down * down + up * up == pytest.approx(s_next * s_next, rel=1e-12)
            want_up = min(s_next, eta * math.sqrt(s_next ** 2 * (s ** 2 - s_next ** 2) / s ** 2))
            assert up == pytest.approx(want_up, rel=1e-12)
    assert all(c[1] == 0.0 for c in euler_ancestral_coefficients(sig, 1.0, 0.0))


@pytest.mark.parametrize("n", [2, 6, 25, 40])
def test_dpmpp_2m_sde_coefficient_identities(n):
    sig = _sigmas(n)
    det = dpmpp_2m_coefficients(sig)
    assert dpmpp_2m_sde_coefficients(sig, 0.0, 1.0) == [c + (0.0,) for c in det], "eta = 0: the 2M tuples themselves"
    for eta, s_noise in ((1.0, 1.0), (0.5, 1.0), (1.0, 0.7)):
        co = dpmpp_2m_sde_coefficients(sig, eta, s_noise)
        assert len(co) == n and co[-1] == (0.0, 1.0, 1.0, 0.0, 0.0) and co[0][2:4] == (1.0, 0.0)
        for i, (a, b, c1, c2, noise) in enumerate(co[:-1]):
            s, s_next = sig[i], sig[i + 1]
            h = math.log(s / s_next)
            assert 0.0 < a < 1.0 and 0.0 < b <= 1.0 and noise > 0.0
            assert a == pytest.approx(s_next / s * math.exp(-eta * h), rel=1e-12)
            assert b == pytest.approx(1.0 - math.exp(-(1.0 + eta) * h), rel=1e-9)
            assert (c1, c2) == (det[i][2], det[i][3])
            # variance bookkeeping: what is left of the old noise plus what is added is the next level
            assert a * a * s * s + (noise / s_noise) ** 2 == pytest.approx(s_next * s_next, rel=1e-12)


def test_coefficient_arguments_are_checked():
    for fn in (euler_ancestral_coefficients, dpmpp_2m_sde_coefficients):
        with pytest.raises(ValueError, match="eta"):
            fn([2.0, 1.0, 0.0], -0.1, 1.0)
        with pytest.raises(ValueError, match="s_noise"):
            fn([2.0, 1.0, 0.0], 1.0, float("nan"))
        with pytest.raises(ValueError, match="decreasing"):
            fn([1.0, 2.0], 1.0, 1.0)


# ------------------------------------------------------------------------------------------------ refusals
def test_entries_refuse_bad_arguments_without_launching():
    """The argument checks of the four new entry points, with no GPU: every call below is refused before anything is
    launched or any pointer is followed (the pointers are made-up addresses)."""
    from vdpp_amd import hip
    lib = hip.load()
    x, e, o, wgt, seeds = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def euler(**kw):
        a = dict(latent=x, eps=e, out=o, sigma=2.0, down=1.0, dims=(1, 3, 4, 4), plan=(3, 3, 1), weights=None, n=0.5,
                 seeds=seeds)
        a.update(kw)
        return lib.sp_euler_ancestral_step_f16(a["latent"], a["eps"], None, 4, None, 0, a["out"], a["sigma"], a["down"], *a["dims"],
                                               *a["plan"], a["weights"], a["n"], a["seeds"], 0, None)

    def sde(**kw):
        a = dict(state=x, eps=e, out=o, sigma=2.0, coef=(0.5, 0.5, 1.0, 0.0), dims=(1, 3, 4, 4), plan=(3, 3, 1), weights=None,
                 n=0.5, seeds=seeds)
        a.update(kw)
        return lib.sp_dpmpp2m_sde_step_f16(a["state"], a["eps"], None, 4, None, 0, a["out"], a["sigma"], *a["coef"], *a["dims"],
                                           *a["plan"], a["weights"], a["n"], a["seeds"], 0, None)

    for fn in (euler, sde):
        for text, kw in (("null seeds", dict(seeds=None)), ("8-byte aligned", dict(seeds=seeds + 4)),
                         ("noise_scale", dict(n=-0.5)), ("noise_scale", dict(n=float("nan"))),
                         ("noise_scale", dict(n=float("inf"))), ("null weights", dict(dims=(1, 5, 4, 4), plan=(3, 2, 2))),
                         ("null weights", dict(plan=(3, 1, 1), dims=(1, 4, 4, 4))), ("n_win", dict(plan=(3, 3, 2), weights=wgt)),
                         ("2^34", dict(dims=(1, 2, 65536, 65536), plan=(2, 2, 1), out=x)),
                         ("sigma", dict(sigma=0.0)), ("null pointer", dict(eps=None))):
            assert fn(**kw) == -1, (fn.__name__, text, kw)
            assert text in lib.sp_last_error().decode(), (fn.__name__, text, lib.sp_last_error())
    assert sde(coef=(1.0, 0.5, 1.0, 0.0)) == -1 and b"a = " in lib.sp_last_error()
    # sp_randn_f16 / sp_philox_blocks_u32
    for text, args in (("null pointer", (None, seeds, 1.0, 1, 3, 4, 4, 0, 0, None)),
                       ("null pointer", (o, None, 1.0, 1, 3, 4, 4, 0, 0, None)),
                       ("aligned", (o + 1, seeds, 1.0, 1, 3, 4, 4, 0, 0, None)),
                       ("aligned", (o, seeds + 2, 1.0, 1, 3, 4, 4, 0, 0, None)),
                       ("dims", (o, seeds, 1.0, 0, 3, 4, 4, 0, 0, None)),
                       ("scale", (o, seeds, -1.0, 1, 3, 4, 4, 0, 0, None)),
                       ("scale", (o, seeds, float("inf"), 1, 3, 4, 4, 0, 0, None)),
                       ("2^34", (o, seeds, 1.0, 1, 2, 65536, 65536, 0, 0, None))):
        assert lib.sp_randn_f16(*args) == -1 and text in lib.sp_last_error().decode(), (text, lib.sp_last_error())
    for text, args in (("null pointer", (None, seeds, 1, 16, 0, 0, None)), ("aligned", (o + 8, seeds, 1, 16, 0, 0, None)),
                       ("dims", (o, seeds, 1, 0, 0, 0, None)), ("2^32", (o, seeds, 1, 2 ** 32 + 1, 0, 0, None))):
        assert lib.sp_philox_blocks_u32(*args) == -1 and text in lib.sp_last_error().decode(), (text, lib.sp_last_error())


# ------------------------------------------------------------------------------------------------ planted mistakes
def _applies(bug, shape, name):
    nb, ft, window, stride, h, w = shape
    if bug == "no_step":
        return name == "history"                       # at step 0 a counter without the step is the right counter
    if bug == "lane_window_local":
        return window != ft and (h * w) % 4 != 0       # with H*W % 4 == 0 the lane does not depend on the frame
    return True


@pytest.mark.parametrize("bug", nm.BUGS)
def test_planted_mistakes_leave_the_step_bound(bug):
    """On the inputs of ``test_noise_gpu.py::test_steps_against_the_fp64_model`` every planted mistake moves an output past
    TWICE the bound the kernels are held to, wherever it is a mistake at all."""
    checked = 0
    for shape in nm.SHAPES:
        for guidance in ("none", "shared", "per-video"):
            for name, st in nm.kernel_steps().items():
                if not _applies(bug, shape, name):
                    continue
                what = (bug, shape, guidance, name)
                if bug != "noise_on_D":
                    lat, ec, eu, g, _ = wm.case_inputs(shape, 8, guidance, channels=4, sigma=st["sigma"])
                    kw = dict(shape=shape, sigma=st["sigma"], **st["euler"])
                    good, terms, nz = nm.euler_ancestral_step(lat, ec, eu, g, nm.SEEDS, st["step"], **kw)
                    bad, _, _ = nm.euler_ancestral_step(lat, ec, eu, g, nm.SEEDS, st["step"], bug=bug, **kw)
                    assert (np.abs(bad - good) / nm.bound(good, terms, nz, shape)).max() > 2.0, what + ("Euler ancestral",)
                if bug != "sigma_up_as_down":
                    state, ec, eu, g, _ = wm.case_inputs(shape, 8, guidance, channels=8, sigma=st["sigma"],
                                                         nan_history=name == "first-order")
                    kw = dict(shape=shape, sigma=st["sigma"], **st["sde"])
                    good_x, good_d, terms, d_terms, nz = nm.dpmpp2m_sde_step(state, ec, eu, g, nm.SEEDS, st["step"], **kw)
                    bad_x, bad_d, _, _, _ = nm.dpmpp2m_sde_step(state, ec, eu, g, nm.SEEDS, st["step"], bug=bug, **kw)
                    if bug == "noise_on_D":
                        assert (np.abs(bad_d - good_d) / nm.bound(good_d, d_terms, 0.0, shape)).max() > 2.0, what + ("2M SDE D",)
                    else:
                        assert (np.abs(bad_x - good_x) / nm.bound(good_x, terms, nz, shape)).max() > 2.0, what + ("2M SDE x'",)
                checked += 1
    assert checked >= 3


# ------------------------------------------------------------------------------------------------ closed-form variance
def _final_variance(sampler, n, s2, eta):
    """Variance of the sample at sigma = 0 for data of variance ``s2`` and the denoiser ``D(x, sigma) = x*s2/(s2 + sigma^2)``:
    every sampler is linear in ``(x_0, z_1 .. z_N)``, independent, of variances ``s2 + sigma_0^2`` and 1, so the sample is a
    row of coefficients over them and the variance the weighted sum of their squares."""
    sig = _sigmas(n)
    x = np.zeros(n + 1)
    x[0] = 1.0
    old = np.zeros(n + 1)
    ea = euler_ancestral_coefficients(sig, eta, 1.0)
    sde = dpmpp_2m_sde_coefficients(sig, eta, 1.0)
    for i in range(n):
        den = x * (s2 / (s2 + sig[i] ** 2))
        if sampler in ("euler", "euler_a"):
            target, noise = (sig[i + 1], 0.0) if sampler == "euler" else ea[i]
            new = x + (x - den) / sig[i] * (target - sig[i])
        else:
            a, b, c1, c2, noise = sde[i] if sampler == "dpmpp_2m_sde" else dpmpp_2m_coefficients(sig)[i] + (0.0,)
            new = a * x + b * (c1 * den - c2 * old)
        new[i + 1] += noise
        x, old = new, den
    var = np.ones(n + 1)
    var[0] = s2 + sig[0] ** 2
    return float((x * x * var).sum())


def _convergence_text():
    lines = ["Variance of the sample at sigma = 0, as a ratio to the data variance s^2 (1 = exact), of the four samplers on",
             "models/euler_schedule.karras_sigma_table(N) with the analytic Gaussian denoiser D(x, sigma) = x*s^2/(s^2 + sigma^2),",
             "x_0 of variance s^2 + sigma_0^2.  Every sampler is linear in (x_0, z_1 .. z_N) there, so the variance follows in",
             "closed form from the host coefficients (models/solver_schedule.py), without sampling; fp64, on the CPU.  Written by",
             "tests/test_noise_cpu.py with SDE_WRITE_CONVERGENCE=1.  Recorded, not asserted: nothing is claimed about which sampler",
             "is better, and nothing about image quality on trained weights.", "",
             f"{'s^2':>6}{'N':>5}{'eta':>6}{'euler':>10}{'euler_a':>10}{'dpmpp_2m':>10}{'2m_sde':>10}"]
    for s2 in (0.25, 1.0, 4.0):
        for n in (13, 25, 50):
            for eta in (0.0, 0.5, 1.0):
                row = [_final_variance(s, n, s2, eta) / s2 for s in ("euler", "euler_a", "dpmpp_2m", "dpmpp_2m_sde")]
                lines.append(f"{s2:>6.2f}{n:>5d}{eta:>6.1f}" + "".join(f"{v:>10.4f}" for v in row))
    return "\n".join(lines) + "\n"


def test_closed_form_variance_table():
    """``eta = 0`` columns are the deterministic samplers' (the same coefficients); the file is what the code gives now."""
    for n in (13, 25):
        assert _final_variance("euler_a", n, 1.0, 0.0) == _final_variance("euler", n, 1.0, 0.0)
        assert _final_variance("dpmpp_2m_sde", n, 1.0, 0.0) == _final_variance("dpmpp_2m", n, 1.0, 0.0)
    text = _convergence_text()
    if os.environ.get("SDE_WRITE_CONVERGENCE") == "1":
        with open(CONVERGENCE, "w") as fh:
            fh.write(text)
    with open(CONVERGENCE) as fh:
        assert fh.read() == text, "profiles/sde_convergence.txt is stale: run this test with SDE_WRITE_CONVERGENCE=1"
