"""The model behind the norm membership tests (tests/norm_model.py), on the CPU:

* the launch plan has the properties csrc/norm.hip relies on, and every GPU case has the seam it was chosen for;
* the kernels' walks, restated, visit every row exactly once;
* every correct fp32 restatement stays within HALF the per-element bound on every GPU case (so the bound is not tight for
  correct code), and the statistics within their own bounds;
* every planted mistake leaves at least TWICE the bound on at least one launch of the sweep the GPU test of its route runs;
* profiles/norm_membership.txt holds these figures (rewritten with NORM_WRITE_MEMBERSHIP=1, stale otherwise).

Sweeps of more than 16 launches are sampled here at eight launches spread over the sweep for the CORRECT restatements (the
GPU test runs all of them); the planted mistakes run the whole sweep of their case."""

import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import norm_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "norm_membership.txt")
GPU_MARK = "---- measured on the MI355X"
G = nm.GROUPS


def _sample(n):
    return list(range(n)) if n <= 16 else sorted({round(i * (n - 1) / 7) for i in range(8)})


_cases = {}


def _case(instances, rows, c):
    key = (instances, rows, c)
    if key not in _cases:
        _cases.clear()                          # one at a time: the largest holds 10 M base values
        _cases[key] = nm.Case(instances, rows, c, G, nm.SEED)
    return _cases[key]


# ---------------------------------------------------------------------------------------------------- plan
def test_plan_properties():
    for instances in (1, 2, 3, 4, 14, 28):
        for c in (64, 256, 320, 640, 960, 1280, 1920, 2560):
            for rows in (1, 37, 144, 300, 576, 1000, 2041, 2304, 4099, 9216, 32256, 129024):
                p = nm.plan(instances, rows, c, G)
                if p["route"] == "fused":
                    assert p["rp"] * p["vpr"] + p["idle"] == 512 and rows <= p["maxit"] * p["rp"]
                    continue
                unit = 4 * p["P"]
                assert p["per"] % unit == 0 and p["rpb"] % unit == 0
                assert 1 <= p["splits"] <= 512 and (p["splits"] - 1) * p["per"] < rows <= p["splits"] * p["per"]
                assert (p["blocks_y"] - 1) * p["rpb"] < rows <= p["blocks_y"] * p["rpb"]
                assert p["fold_in_apply"] == (p["splits"] <= 128)
    for c, rp in ((256, 512), (1280, 102), (2560, 51)):
        assert [nm.plan(1, r, c, G).get("maxit") for r in (16 * rp, 16 * rp + 1, 20 * rp, 20 * rp + 1)] == [16, 20, 20, None]


def test_every_case_has_the_seam_it_was_chosen_for():
    p = nm.plan(2, 300, 320, G)
    assert (p["route"], p["splits"], p["fold_in_apply"], p["blocks_y"]) == ("split", 1, True, 2)
    p = nm.plan(2, 1000, 320, G)                   # the last split is the tail loop alone: 40 rows < 4 P = 48
    assert (p["per"], p["splits"], 1000 - 4 * p["per"], p["P"]) == (240, 5, 40, 12)
    p = nm.plan(3, 1000, 640, G)
    assert p["route"] == "split" and p["splits"] > 1 and 1000 % p["per"] != 0 and 1000 % p["rpb"] != 0
    p = nm.plan(1, 4099, 2560, G)                  # more than 128 splits: gn_finalize_kernel, ragged last split
    assert (p["per"], p["splits"], p["fold_in_apply"], 4099 % p["per"]) == (20, 205, False, 19)
    for case, maxit, vpr, idle in (((4, 200, 256), 16, 1, 0), ((1, 8192, 256), 16, 1, 0), ((1, 1632, 1280), 16, 5, 2),
                                   ((1, 1633, 1280), 20, 5, 2), ((1, 2040, 1280), 20, 5, 2), ((1, 1020, 2560), 20, 10, 2)):
        p = nm.plan(*case, G)
        assert (p["route"], p["maxit"], p["vpr"], p["idle"]) == ("fused", maxit, vpr, idle), case
    assert nm.plan(1, 2041, 1280, G)["route"] == "split" and nm.launches(1, 2041) >= 3
    # two instances of 1,020 x 2,560 are 10.4 MB in 64 slabs: neither rule of the fused route holds, three launches
    assert nm.plan(2, 1020, 2560, G)["route"] == "split"
    assert nm.tile_plan(1, 33280, 64, G)["records"] == 260
    p = nm.plan(*nm.LARGE_CASE, G)                 # several thousand rows: 7 splits of 5 batches, then one batch + 3 tail rows
    assert (p["route"], p["P"], p["per"], p["splits"], 9219 - 7 * p["per"] - 4 * p["P"]) == ("split", 64, 1280, 8, 3)
    # the seam at 24 of 64 channels lies between two-channel groups; the seam at 20 of 256 lies inside group 2
    assert 24 % (64 // G) == 0 and 20 % (256 // G) == 4 and (2, 512, 64, 24) in nm.TILE_CASES and (2, 512, 256, 20) in nm.TILE_CASES
    for rows, c in nm.LN_WIDTHS:
        assert rows >= c and rows % 4 != 0
    assert sorted({nm.ln_plan(r, c, False)["nv"] for r, c in nm.LN_WIDTHS}) == [1, 2, 3, 4]
    assert {(c // 8) % 64 == 0 for _, c in nm.LN_WIDTHS} == {True, False}
    assert [nm.ln_plan(r, c, True)["kernel"] for r, c in nm.LN_ROWS_CASES] == \
        ["ln_stats", "ln_stats_rows", "ln_stats_rows", "ln_stats_rows", "ln_stats_rows"]
    for c, thr in ((320, 8192), (640, 4096), (1280, 2048)):
        assert [nm.ln_plan(r, c, True)["kernel"] for r in (thr - 1, thr)] == ["ln_stats", "ln_stats_rows"]


def test_walks_visit_every_row_once():
    for instances, rows, c in nm.GN_SPLIT_CASES:
        p = nm.plan(instances, rows, c, G)
        for per, blocks in ((p["per"], p["splits"]), (p["rpb"], p["blocks_y"])):
            m = nm.row_walk(rows, p["P"], per, blocks)
            assert (m[:rows] == 1).all() and m[rows:].sum() == 0
    for instances, rows, c in nm.GN_FUSED_CASES:
        p = nm.plan(instances, rows, c, G)
        row, q, live = nm.fused_walk(rows, p["vpr"], p["maxit"])
        seen = np.zeros((rows, p["vpr"]), dtype=int)
        np.add.at(seen, (row[live], np.broadcast_to(q[None, :], row.shape)[live]), 1)
        assert (seen == 1).all()


def test_one_generator_for_numpy_and_torch():
    ar = lambda n: torch.arange(n, dtype=torch.int64)
    for sr in (nm.row_spike, nm.record_spike):
        a = nm.spike_values(np, nm._ar, 2, 256, 64, G, 3, nm.SEED, 40, sr)
        b = nm.spike_values(torch, ar, 2, 256, 64, G, 3, nm.SEED, 40, sr)
        assert np.array_equal(a, b.numpy())
    assert np.array_equal(nm.ln_values(np, nm._ar, 70, 64, 1, 40), nm.ln_values(torch, ar, 70, 64, 1, 40).numpy())
    assert np.array_equal(nm.ln_addvec(nm._ar, 3, 64, 1), nm.ln_addvec(ar, 3, 64, 1).numpy())
    for u, v in zip(nm.affine(nm._ar, 320), nm.affine(ar, 320)):
        assert np.array_equal(u, v.double().numpy()) and np.array_equal(u, u.astype(np.float32))


def test_the_device_arithmetic_is_the_models():
    """tests/test_norm_membership_gpu.py restates the statistics, the reference and the bound in torch: held to this file here"""
    from tests import test_norm_membership_gpu as dev
    inst, rows, c = 2, 300, 320
    s = nm.Slabs(_case(inst, rows, c), 1, 40)
    xi = torch.from_numpy(s.x)
    mean, rstd = dev.slab_stats(xi, inst, rows, c)
    assert np.array_equal(mean.numpy(), s.mean) and np.allclose(rstd.numpy(), s.rstd, rtol=1e-15, atol=0)
    g = np.arange(c) // (c // G)
    for silu in (0, 1):
        want = nm.reference(s.x.reshape(inst, rows, c).astype(np.float64), s.mean[:, None, g], s.rstd[:, None, g], s.gamma, s.beta,
                            silu, 134)
        got = dev.reference(xi.double().view(inst, rows, c), torch.from_numpy(s.mean[:, None, g]), torch.from_numpy(s.rstd[:, None, g]),
                            torch.from_numpy(s.gamma), torch.from_numpy(s.beta), silu, 134)
        for a, b in zip(got, want):
            assert np.allclose(a.numpy(), b, rtol=1e-12, atol=0)
    v = np.array([0.0, 1e-9, 2.0 ** -14, 0.999, 1.0, 1.5, 2.0, -37.25, 6.0e4])
    assert np.array_equal(dev.ulp16(torch.from_numpy(v)).numpy(), nm.ulp16(v))
    assert np.array_equal(nm.ulp16(v), [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -5, 32.0])


def test_the_spike_design():
    inst, rows, c = 2, 300, 320
    cs = _case(inst, rows, c)
    seen = np.zeros(rows, dtype=int)
    for l in range(nm.launches(inst, rows)):
        s = nm.Slabs(cs, l, 40)
        x = nm.spike_slabs(inst, rows, c, G, l, nm.SEED, 40).astype(np.int64)
        assert np.array_equal(x, s.x)                                         # the row-sum form is the same data
        mean, var, rstd = nm.slab_stats(x, inst, rows, c, G)
        assert np.array_equal(mean, s.mean) and np.array_equal(rstd, s.rstd)
        xg = x.reshape(inst, rows, G, c // G) - s.off[:, None, :, None]
        for i in range(inst):
            for g in range(G):
                (at,) = np.nonzero(np.abs(xg[i, :, g]).max(1) > 2)
                assert len(at) == 1 and at[0] == s.srow[i, g]                 # one spike row per slab
                seen[at[0]] += 1
                row, first = xg[i, at[0], g], xg[i, 0, g, 0]
                # at least two values, none of them the shift reference (which stays a base value)
                assert len(set(row[1:])) >= 2 and abs(first) <= 2 and (row[1:] != first).all()
    # the sweep puts the spike on every row index once, in one of the instances (the walks do not depend on the instance)
    assert (seen >= 1).all() and seen.sum() == nm.launches(inst, rows) * inst * G


# ---------------------------------------------------------------------------------------------------- clean margins
@functools.lru_cache(maxsize=None)
def _gn_margin(case):
    cs = _case(*case)
    worst = 0.0
    for l in _sample(nm.launches(case[0], case[1])):
        for silu, off in nm.COMBOS:
            worst = max(worst, nm.gn(nm.Slabs(cs, l, off), silu)["factor"])
    return worst


@functools.lru_cache(maxsize=None)
def _tile_margin(case):
    inst, rows, c, c_a = case
    cs = _case(inst, rows, c)
    worst = st_worst = 0.0
    for l in _sample(rows // nm.HALF_TILE):
        for silu, off in nm.COMBOS:
            s = nm.Slabs(cs, l, off, nm.record_spike)
            out = nm.gn_tile_sums(s, silu, c_a)
            worst = max(worst, out["factor"])
            st_worst = max(st_worst, _tile_stats_ratio(s, out["stats"]))
    return worst, st_worst


def _tile_stats_ratio(s, stats):
    ulp, rel = nm.tile_stats_bounds(s.mean)
    return max(float((np.abs(stats[..., 0].astype(np.float64) - s.mean) / ulp).max()),
               float((np.abs(stats[..., 1].astype(np.float64) / s.rstd - 1.0) / rel).max()))


@functools.lru_cache(maxsize=None)
def _ln_margin(rows, c, stats_only, add):
    p = nm.ln_plan(rows, c, stats_only)
    out = dict(mean=0.0, rstd=0.0, y=0.0)
    for off in (0, 40):
        r = nm.Rows(rows, c, nm.SEED, off, nm.ADDVEC_ROWS if add else 0)
        if p["kernel"] == "ln_stats_rows":
            xs, mean32, rstd32, stored = nm.ln_rows_per_wave(r, p["lpr"])
        else:
            xs, mean32, rstd32 = nm.ln_wave_per_row(r)
            stored = rows
        res = nm.ln_check(r, xs, mean32, rstd32, not stats_only, stored)
        assert res["sum_equal"] and res["guard_ok"]
        out = {k: max(out[k], res[k]) for k in out}
    return out


@pytest.mark.parametrize("case", nm.GN_SPLIT_CASES + nm.GN_FUSED_CASES)
def test_correct_groupnorm_restatements_stay_within_half_the_bound(case):
    assert _gn_margin(case) <= 0.5


@pytest.mark.parametrize("case", nm.TILE_CASES)
def test_correct_tile_sums_restatements_stay_within_half_the_bound(case):
    worst, st = _tile_margin(case)
    assert worst <= 0.5 and st <= 1.0


@pytest.mark.parametrize("rows,c", nm.LN_WIDTHS)
def test_correct_layernorm_restatements_stay_within_half_the_bound(rows, c):
    for stats_only in (False, True):
        for add in (False, True):
            m = _ln_margin(rows, c, stats_only, add)
            assert m["y"] <= 0.5 and m["mean"] <= 1.0 and m["rstd"] <= 0.5, m


@pytest.mark.parametrize("rows,c", nm.LN_ROWS_CASES)
def test_correct_rows_per_wave_restatements_stay_within_the_statistics_bounds(rows, c):
    for add in (False, True):
        m = _ln_margin(rows, c, True, add)
        assert m["mean"] <= 1.0 and m["rstd"] <= 0.5, m


# ---------------------------------------------------------------------------------------------------- planted mistakes
def _old_check_accepts(res):
    return res["rel_l2"] <= 2e-3 and res["max_rel"] <= 1e-2


def _run_mistake(name, case=None):
    """-> (largest factor over the bound in the sweeps at offsets 0 and 40, launches that reach 2 x / launches, and what check()
    of tests/test_kernels_gpu.py measures on the launch at offset 0 where the mistake shows LEAST -- there the rows it touches
    are ordinary ones, as all rows are on check()'s Gaussian data)"""
    route, own, kind = nm.MISTAKES[name]
    case = case or own
    results = {0: [], 40: []}
    if route in ("split", "fused"):
        cs = _case(*case)
        for off in results:
            for l in range(nm.launches(case[0], case[1])):
                results[off].append(nm.gn(nm.Slabs(cs, l, off), 0, name))
    elif route == "tile_sums":
        inst, rows, c, c_a = case
        cs = _case(inst, rows, c)
        for off in results:
            for l in range(rows // nm.HALF_TILE):
                results[off].append(nm.gn_tile_sums(nm.Slabs(cs, l, off, nm.record_spike), 0, c_a, name))
    else:
        rows, c = case
        r = nm.Rows(rows, c, nm.SEED, 40, nm.ADDVEC_ROWS)
        if route == "ln":
            xs, mean32, rstd32 = nm.ln_wave_per_row(r, name)
            stored = rows
        else:
            xs, mean32, rstd32, stored = nm.ln_rows_per_wave(r, nm.ln_plan(rows, c, True)["lpr"], name)
        res = nm.ln_check(r, xs, mean32, rstd32, route == "ln", stored)
        f = max(res["mean"], 0.5 * res["rstd"], res["y"])            # rstd is held to 2^-18: half of it is "the bound" here
        if not (res["sum_equal"] and res["guard_ok"]):
            f = math.inf
        return dict(factor=f, caught=1, launches=1, check=None)
    least = min(results[0], key=lambda d: d["factor"])
    both = results[0] + results[40]
    check = None if math.isinf(least["factor"]) else (least["rel_l2"], least["max_rel"], _old_check_accepts(least))
    return dict(factor=max(d["factor"] for d in both), caught=sum(d["factor"] >= 2.0 for d in both), launches=len(both),
                check=check)                      # (rows left unwritten hold whatever the buffer held: nothing to measure)


@pytest.fixture(scope="module")
def mistakes():
    out = {name: _run_mistake(name) for name in nm.MISTAKES}
    out.update({(name, nm.LARGE_CASE): _run_mistake(name, nm.LARGE_CASE) for name in nm.LARGE_MISTAKES})
    return out


def test_there_are_at_least_twelve_planted_mistakes():
    assert len(nm.MISTAKES) >= 12


@pytest.mark.parametrize("name", list(nm.MISTAKES))
def test_every_planted_mistake_leaves_twice_the_bound(mistakes, name):
    assert mistakes[name]["factor"] >= 2.0 and mistakes[name]["caught"] >= 1


def test_what_the_older_yardstick_makes_of_the_mistakes(mistakes):
    """With the touched rows ordinary ones, as on check()'s Gaussian data, the two idle threads' vectors counted twice
    (15 rows x 16 channels of a 1,632 x 40 slab) stay inside check()'s relative L2 of 2e-3 and maximum of 1e-2; so does no
    mistake that the new bound misses.  (The shapes here are the smallest with each seam, a few hundred rows, where a whole
    tail or a wrong count is coarse enough for check() as well: the table in profiles/norm_membership.txt has every figure.)"""
    assert mistakes["fused_idle_threads_live"]["check"][2]
    assert all(m["factor"] >= 2.0 for m in mistakes.values())
    # at 9,219 rows the statistics mistakes of the split route are invisible to check() as well, wherever the spike is not
    # on one of their rows, and the moving spike still finds them
    for name in nm.LARGE_MISTAKES:
        m = mistakes[(name, nm.LARGE_CASE)]
        assert m["check"][2] and m["factor"] >= 2.0, (name, m)


# ---------------------------------------------------------------------------------------------------- the record
def _fmt(v):
    return "inf" if math.isinf(v) else f"{v:.3g}"


def _record(mistakes):
    lines = ["Norm membership tests: tests/norm_model.py, tests/test_norm_membership_cpu.py, tests/test_norm_membership_gpu.py.",
             "Written by tests/test_norm_membership_cpu.py with NORM_WRITE_MEMBERSHIP=1 (down to the MI355X section, which is kept);",
             "the test fails when it is stale.  All factors are worst |y - ref| / bound over every element, bound = one fp16 ulp of",
             "the fp64 reference + 16 * 2^-24 * (|x sc| + |mean sc| + |beta|).",
             "",
             "Correct fp32 restatements (must stay <= 0.5; SiLU on and off, offsets 0 and +-40; sweeps of more than 16 launches",
             "sampled at 8):",
             "",
             f"{'case':28s} {'route':10s} {'launches':>8s}  worst"]
    for case in nm.GN_SPLIT_CASES + nm.GN_FUSED_CASES:
        lines.append(f"{str(case):28s} {nm.plan(*case, G)['route']:10s} {nm.launches(case[0], case[1]):8d}  {_gn_margin(case):.3f}")
    for case in nm.TILE_CASES:
        worst, st = _tile_margin(case)
        lines.append(f"{str(case):28s} {'tile_sums':10s} {case[1] // nm.HALF_TILE:8d}  {worst:.3f}   statistics {st:.2f} of their bounds")
    lines += ["", "LayerNorm (mean / one fp32 ulp of max|x|, rstd / 2^-18, y / bound; with and without the pre-add, offsets 0 and 40):", ""]
    for rows, c in nm.LN_WIDTHS:
        a, b = _ln_margin(rows, c, False, True), _ln_margin(rows, c, True, True)
        lines.append(f"{str((rows, c)):28s} ln<{nm.ln_plan(rows, c, False)['nv']}>      mean {max(a['mean'], b['mean']):.2f}  "
                     f"rstd {max(a['rstd'], b['rstd']):.3f}  y {a['y']:.3f}")
    for rows, c in nm.LN_ROWS_CASES:
        p = nm.ln_plan(rows, c, True)
        m = _ln_margin(rows, c, True, True)
        kern = f"rows<{p['lpr']},2>" if p["kernel"] == "ln_stats_rows" else f"ln_stats<{p['nv']}>"
        lines.append(f"{str((rows, c)):28s} {kern:10s} mean {m['mean']:.2f}  rstd {m['rstd']:.3f}")
    lines += ["", "Planted mistakes (SiLU off, the whole sweep of the case at offsets 0 and 40; must reach >= 2).  check(): what the older",
              "yardstick of tests/test_kernels_gpu.py (relative L2 <= 2e-3, max <= 1e-2 max|ref|) measures on the launch at offset 0",
              "where the mistake shows least, i.e. where the rows it touches are ordinary ones as on check()'s Gaussian data",
              "(base-value weights taken from the case without its spike rows).",
              "",
              f"{'mistake':30s} {'case':22s} {'kind':11s} {'factor':>9s} {'caught':>9s}   check(): rel_l2   max_rel  verdict"]
    for name, (route, case, kind) in nm.MISTAKES.items():
        m = mistakes[name]
        chk = "-" if m["check"] is None else f"{m['check'][0]:.1e}  {m['check'][1]:.1e}  {'accepts' if m['check'][2] else 'rejects'}"
        lines.append(f"{name:30s} {str(case):22s} {kind:11s} {_fmt(m['factor']):>9s} {m['caught']:4d}/{m['launches']:<4d}   {chk}")
    lines += ["", "The same at several thousand rows (eight splits, the last of 259 rows: one batch and a tail of three), where the",
              "touched rows are 8 and 3 of 9,219 -- check() accepts both on every launch that has no spike on those rows:", ""]
    for name in nm.LARGE_MISTAKES:
        m = mistakes[(name, nm.LARGE_CASE)]
        chk = f"{m['check'][0]:.1e}  {m['check'][1]:.1e}  {'accepts' if m['check'][2] else 'rejects'}"
        lines.append(f"{name:30s} {str(nm.LARGE_CASE):22s} {'statistics':11s} {_fmt(m['factor']):>9s} {m['caught']:4d}/{m['launches']:<4d}   {chk}")
    return "\n".join(lines) + "\n\n"


def test_record_file(mistakes):
    text = _record(mistakes)
    tail = ""
    if os.path.exists(RECORD):
        with open(RECORD) as fh:
            old = fh.read()
        if GPU_MARK in old:
            tail = old[old.index(GPU_MARK):]
    if os.environ.get("NORM_WRITE_MEMBERSHIP") == "1":
        with open(RECORD, "w") as fh:
            fh.write(text + tail)
    with open(RECORD) as fh:
        got = fh.read()
    assert got.split(GPU_MARK)[0] == text, "profiles/norm_membership.txt is stale: run this test with NORM_WRITE_MEMBERSHIP=1"
