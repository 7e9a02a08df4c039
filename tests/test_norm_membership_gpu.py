"""csrc/norm.hip held per element: every row and channel counted once (tests/norm_model.py has the design and the bound).

Every test makes its input on the device by index arithmetic (small integers in fp16 with one moving spike row per slab),
takes the exact statistics from integer sums in torch.float64 there, compares there, and brings back only the worst
|got - ref| / bound with its place.  Outputs lie between guard rows pre-filled with NaN: the output must be finite and
within the bound, the guards untouched.  Every case first asserts, through norm_model.plan, the route and partition it was
written for.  tests/test_norm_membership_cpu.py shows that correct fp32 arithmetic stays within half of these bounds and
that fifteen planted mistakes leave at least twice the bound."""

import math

import pytest
import torch

from tests import norm_model as nm

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = nm.GROUPS
GUARD = 4                   # NaN rows on either side of an output
EXTRA = 24                  # foreign columns in front of x in the strided call


def _ops():
    from vdpp_amd.hip import ops
    return ops


def _ar(n):
    return torch.arange(n, dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------ the model's arithmetic in torch
def ulp16(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 10)


def reference(x, mean, rstd, gamma, beta, silu, sum_terms=0):
    """norm_model.reference on fp64 tensors"""
    sc = rstd * gamma
    pre = (x - mean) * sc + beta
    slack = nm.BOUND_K * nm.U * ((x * sc).abs() + (mean * sc).abs() + beta.abs()) + sum_terms * nm.U * ((x - mean) * sc).abs()
    if silu:
        ref = pre / (1.0 + torch.exp(-pre))
        return ref, ulp16(ref) + 1.1 * slack
    return pre, ulp16(pre) + slack


def exact_stats(s1, s2, n, eps):
    """norm_model._exact on int64 tensors"""
    mean = s1.double() / float(n)
    var = (n * s2 - s1 * s1).double() / float(n) / float(n)
    return mean, 1.0 / torch.sqrt(var + eps)


def slab_stats(xi, instances, rows, c):
    x4 = xi.view(instances, rows, G, c // G)
    return exact_stats(x4.sum(dim=(1, 3)), (x4 * x4).sum(dim=(1, 3)), rows * (c // G), nm.EPS_GN)


def worst_ratio(got, ref, bnd):
    """(worst |got - ref| / bound with NaN counted as infinite, its flat index) as a 2-vector on the device"""
    ratio = torch.nan_to_num(((got.double() - ref).abs() / bnd), nan=math.inf, posinf=math.inf).flatten()
    mx, at = ratio.max(0)
    return torch.stack([mx, at.double()])


def guarded(rows, cols, dtype=torch.float16):
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf, rows):
    return (torch.isnan(buf[:GUARD]).all() & torch.isnan(buf[GUARD + rows:]).all()).double().reshape(1)


class Sweep:
    """collects one record per launch on the device; one transfer at the end"""

    def __init__(self, what):
        self.what, self.recs, self.tags = what, [], []

    def add(self, tag, *parts):
        self.recs.append(torch.cat([p.reshape(-1).double() for p in parts]))
        self.tags.append(tag)

    def finish(self, cols, names, limits):
        """names / limits: of the leading columns that are ratios; the remaining columns are flags that must be 1.
        cols: the row length of the checked tensor (to name instance-row and channel)"""
        r = torch.stack(self.recs).cpu()
        k = len(names)
        report = []
        for j, (name, lim) in enumerate(zip(names, limits)):
            col = r[:, 2 * j]
            i = int(col.argmax())
            at = int(r[i, 2 * j + 1])
            report.append(f"{name} {float(col[i]):.3f}")
            assert float(col[i]) <= lim, (f"{self.what}: {name} is {float(col[i]):.3f} of its bound at launch {self.tags[i]}, "
                                          f"row {at // cols[j]}, channel {at % cols[j]}")
        flags = r[:, 2 * k:]
        bad = (flags != 1).any(1).nonzero().flatten().tolist()
        assert not bad, f"{self.what}: guard rows touched / outputs differ at launches {[self.tags[i] for i in bad[:4]]}"
        print(f"norm-membership {self.what}: {len(self.recs)} launches, worst " + ", ".join(report))


def _expand(t, rows, cpg):
    """[instances][groups] -> [instances * rows][c]"""
    return t.repeat_interleave(cpg, 1).repeat_interleave(rows, 0)


# ------------------------------------------------------------------------------------------ GroupNorm
GN = [  # (instances, rows, c), what plan() must say
    ((2, 300, 320), dict(route="split", splits=1, fold_in_apply=True, blocks_y=2)),
    ((2, 1000, 320), dict(route="split", per=240, splits=5, fold_in_apply=True)),            # last split: 40 rows, the tail loop
    ((3, 1000, 640), dict(route="split", per=120, splits=9, rpb=96, blocks_y=11)),
    ((1, 4099, 2560), dict(route="split", per=20, splits=205, fold_in_apply=False)),         # gn_finalize_kernel
    ((4, 200, 256), dict(route="fused", maxit=16, vpr=1, idle=0)),
    ((1, 8192, 256), dict(route="fused", maxit=16, vpr=1, rp=512)),
    ((1, 1632, 1280), dict(route="fused", maxit=16, vpr=5, rp=102, idle=2)),
    ((1, 1633, 1280), dict(route="fused", maxit=20, vpr=5, rp=102, idle=2)),
    ((1, 2040, 1280), dict(route="fused", maxit=20, vpr=5, rp=102, idle=2)),
    ((1, 2041, 1280), dict(route="split", splits=35, fold_in_apply=True)),                    # just past the fused range
    ((2, 1020, 2560), dict(route="split", per=20, splits=51)),                                # 10.4 MB in 64 slabs: not fused
    ((1, 1020, 2560), dict(route="fused", maxit=20, vpr=10, rp=51, idle=2)),                  # ten vectors per row
    ((1, 9219, 64), dict(route="split", P=64, per=1280, splits=8, fold_in_apply=True)),       # thousands of rows: where check() is blind
]


@pytest.mark.parametrize("case,want", GN, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c, _ in GN])
def test_groupnorm_counts_every_row_once(case, want):
    """sp_groupnorm_f16 / sp_groupnorm_ld_f16: the whole sweep (the spike on every row index once) with SiLU on and off and
    group offsets 0 and +-40; on the first launch of every combination the strided call (foreign columns 3.0e4) must give the
    dense call's bytes."""
    ops = _ops()
    inst, rows, c = case
    p = nm.plan(inst, rows, c, G)
    assert {k: p[k] for k in want} == want and sorted(nm.GN_SPLIT_CASES + nm.GN_FUSED_CASES) == sorted(c for c, _ in GN)
    R, cpg = inst * rows, c // G
    gamma, beta = (t.double() for t in nm.affine(_ar, c))
    g32, b32 = gamma.float(), beta.float()
    ws = torch.empty(ops.groupnorm_ws_bytes(inst, rows, c, G), dtype=torch.uint8, device=DEV)
    kw = dict(instances=inst, rows=rows, c=c, groups=G, eps=1e-6, ws=ws)
    buf, y = guarded(R, c)
    sweep = Sweep(f"groupnorm {case} {p['route']}")
    for silu, off in nm.COMBOS:
        for l in range(nm.launches(inst, rows)):
            xi = nm.spike_values(torch, _ar, inst, rows, c, G, l, nm.SEED, off)
            x = xi.half()
            buf.fill_(float("nan"))
            ops.groupnorm(x, g32, b32, y, silu=silu, **kw)
            mean, rstd = slab_stats(xi, inst, rows, c)
            ref, bnd = reference(xi.double(), _expand(mean, rows, cpg), _expand(rstd, rows, cpg), gamma[None, :], beta[None, :],
                                 silu, nm.sum_terms(p))
            same = torch.ones(1, device=DEV)
            if l == 0:
                wide = torch.full((R, c + EXTRA), 3.0e4, dtype=torch.float16, device=DEV)
                wide[:, EXTRA:] = x
                y2 = torch.empty(R, c, dtype=torch.float16, device=DEV)
                ops.groupnorm(wide[:, EXTRA:], g32, b32, y2, silu=silu, ldx=c + EXTRA, **kw)
                same = (y2.view(torch.int16) == y.view(torch.int16)).all().reshape(1)
            sweep.add((l, silu, off), worst_ratio(y, ref, bnd), guards_intact(buf, R), same)
    sweep.finish([c], ["y"], [1.0])


def test_the_comparison_resolves_one_ordinary_row():
    """The yardstick itself, on the real kernel: hand sp_groupnorm_f16 an input in which ONE ordinary row of a 300-row instance
    is replaced by its neighbour (for the statistics: one row dropped, one counted twice) and compare every OTHER row with the
    reference of the intact input -- the per-element bound must be broken at least twofold, where check()'s 2e-3 sees nothing."""
    ops = _ops()
    inst, rows, c, cpg = 2, 300, 320, 10
    xi = nm.spike_values(torch, _ar, inst, rows, c, G, 0, nm.SEED, 0)
    row = rows + 150                                             # instance 1, whose spikes of launch 0 sit on rows 32 .. 63
    assert int((xi[row].abs().max())) <= 2 and int((xi[row - 1].abs().max())) <= 2
    gamma, beta = (t.double() for t in nm.affine(_ar, c))
    ws = torch.empty(ops.groupnorm_ws_bytes(inst, rows, c, G), dtype=torch.uint8, device=DEV)
    mean, rstd = slab_stats(xi, inst, rows, c)
    ref, bnd = reference(xi.double(), _expand(mean, rows, cpg), _expand(rstd, rows, cpg), gamma[None, :], beta[None, :], 0)
    keep = torch.ones(inst * rows, dtype=torch.bool, device=DEV)
    keep[row] = False
    worst = []
    for damaged in (False, True):
        x = xi.clone()
        if damaged:
            x[row] = x[row - 1]
        buf, y = guarded(inst * rows, c)
        ops.groupnorm(x.half(), gamma.float(), beta.float(), y, instances=inst, rows=rows, c=c, groups=G, eps=1e-6, silu=0, ws=ws)
        worst.append(worst_ratio(y[keep], ref[keep], bnd[keep])[0])
        out = y.float()
        worst.append(((out[keep] - ref[keep].float()).norm() / ref[keep].float().norm()).double())
    clean, _, broken, l2 = (float(v) for v in torch.stack(worst).cpu())
    print(f"norm-membership one ordinary row of 300 replaced: {broken:.1f} of the bound (intact {clean:.3f}), relative L2 {l2:.1e}")
    assert clean <= 1.0 and broken >= 2.0 and l2 <= 2e-3


# ------------------------------------------------------------------------------------------ tile sums
def _tile_inputs(xi, c, c_a):
    """exact half-tile column sums of the integer input, as a contraction's epilogue leaves them: [tile][half][c][2] fp32"""
    xr = xi.view(-1, nm.HALF_TILE, c)
    part = torch.stack([xr.sum(1), (xr * xr).sum(1)], dim=-1).float().contiguous()
    if c_a is None:
        return part, None
    return part[:, :c_a].contiguous(), part[:, c_a:].contiguous()


def _stats_ratios(stats, mean, rstd):
    """returned (mean, rstd) against the closed form: the mean within one fp32 ulp, rstd within 2^-22 relative"""
    st = stats.view(-1, 2).double()
    m, r = mean.reshape(-1), rstd.reshape(-1)
    ulp = torch.exp2(torch.floor(torch.log2(m.abs().clamp_min(2.0 ** -126))) - 23)      # of the mean's own binade
    return worst_ratio(st[:, 0], m, ulp), worst_ratio(st[:, 1] / r, torch.ones_like(r), torch.full_like(r, 2.0 ** -22))


@pytest.mark.parametrize("inst,rows,c,c_a", nm.TILE_CASES, ids=["2x512", "1x33280_stride_256", "2x512_seam_between_groups",
                                                                "2x512x256_seam_inside_a_group"])
def test_groupnorm_from_tile_sums_counts_every_record_once(inst, rows, c, c_a):
    """sp_groupnorm_tile_sums_f16 / _tile_sums2_f16 on synthesised sums (no contraction): the spike through every half-tile
    record; 260 records cross the finalize kernel's stride of 256.  Two seams: c_a = 24 of 64 channels lies between the
    two-channel groups 11 and 12 (every group reads one producer, with that producer's pitch); c_a = 20 of 256 channels
    lies inside group 2 (channels 16 .. 23), which takes four channels from each producer -- a kernel that chose the producer
    once per group would read the wrong four."""
    ops = _ops()
    p = nm.tile_plan(inst, rows, c, G)
    assert p["records"] == rows // 128 and (p["records"] > 256) == (rows == 33280) and p["rpb"] % (4 * p["P"]) == 0
    if c_a is not None:
        assert (c_a % (c // G) != 0) == (c == 256) and c_a % 4 == 0 and (c - c_a) % 4 == 0
    R, cpg = inst * rows, c // G
    gamma, beta = (t.double() for t in nm.affine(_ar, c))
    g32, b32 = gamma.float(), beta.float()
    buf, y = guarded(R, c)
    sbuf, stats = guarded(inst * G, 2, torch.float32)
    sweep = Sweep(f"tile_sums {(inst, rows, c, c_a)}")
    for silu, off in nm.COMBOS:
        for l in range(p["records"]):
            xi = nm.spike_values(torch, _ar, inst, rows, c, G, l, nm.SEED, off, nm.record_spike)
            pa, pb = _tile_inputs(xi, c, c_a)
            buf.fill_(float("nan"))
            sbuf.fill_(float("nan"))
            ops.groupnorm_tile_sums(xi.half(), pa, g32, b32, y, instances=inst, rows=rows, c=c, groups=G, eps=1e-6, silu=silu,
                                    stats=stats, part_b=pb, c_a=c_a)
            mean, rstd = slab_stats(xi, inst, rows, c)
            ref, bnd = reference(xi.double(), _expand(mean, rows, cpg), _expand(rstd, rows, cpg), gamma[None, :], beta[None, :], silu)
            sweep.add((l, silu, off), worst_ratio(y, ref, bnd), *_stats_ratios(stats, mean, rstd), guards_intact(buf, R),
                      guards_intact(sbuf, inst * G))
    sweep.finish([c, 1, 1], ["y", "mean", "rstd"], [1.0, 1.0, 1.0])


@pytest.mark.parametrize("inst,rows,c", [(2, 512, 64), (1, 33280, 64)])
def test_groupnorm_folded_linear_from_tile_sums(inst, rows, c):
    """sp_groupnorm_fold_linear_tile_sums_f16: w_out within one fp16 ulp of w * gamma * rstd in fp64 from the closed-form
    statistics, bias_out = sum(beta w - mean w_out) + bias from the ROUNDED weights it stored (norm_model.fold_linear_reference)"""
    ops = _ops()
    n, cpg, recs = 40, c // G, rows // 128                      # 40 output rows: a ragged second block of 32
    gamma, beta = (t.double() for t in nm.affine(_ar, c))
    idx = _ar(n)[:, None] * c + _ar(c)[None, :]
    w = (nm._base(idx, 11).double() / 4.0 + (idx % 7).double() / 64.0)
    bias = ((_ar(n) * 29) % 31 - 15).double() / 8.0
    wbuf, w_out = guarded(inst * n, c)
    bbuf, b_out = guarded(inst, n, torch.float32)
    sbuf, stats = guarded(inst * G, 2, torch.float32)
    g = _ar(c) // cpg
    sweep = Sweep(f"fold_linear_tile_sums {(inst, rows, c)}")
    for off in (0, 40):
        for l in range(recs):                                   # the spike through every half-tile record
            xi = nm.spike_values(torch, _ar, inst, rows, c, G, l, nm.SEED, off, nm.record_spike)
            part, _ = _tile_inputs(xi, c, None)
            for b in (wbuf, bbuf, sbuf):
                b.fill_(float("nan"))
            ops.groupnorm_fold_linear_tile_sums(part, gamma.float(), beta.float(), w.half(), bias.float(), w_out.view(inst, n, c),
                                                b_out, instances=inst, rows=rows, c=c, groups=G, eps=1e-6, n=n, stats=stats)
            mean, rstd = slab_stats(xi, inst, rows, c)
            w_ref = w[None] * (gamma[None, :] * rstd[:, g])[:, None, :]
            wq = w_out.view(inst, n, c).double()
            b_ref = (beta[None, None, :] * w[None] - mean[:, g][:, None, :] * wq).sum(-1) + bias[None, :]
            mag = ((beta[None, None, :] * w[None]).abs() + (mean[:, g][:, None, :] * wq).abs()).sum(-1) + bias.abs()[None, :]
            sweep.add((l, off), worst_ratio(wq, w_ref, ulp16(w_ref)), worst_ratio(b_out, b_ref, nm.fold_bias_units(c) * nm.U * mag),
                      *_stats_ratios(stats, mean, rstd), guards_intact(wbuf, inst * n), guards_intact(bbuf, inst),
                      guards_intact(sbuf, inst * G))
    sweep.finish([c, n, 1, 1], ["w_out", "bias_out", "mean", "rstd"], [1.0, 1.0, 1.0, 1.0])


# ------------------------------------------------------------------------------------------ LayerNorm
def _ln_inputs(rows, c, off, add):
    xi = nm.ln_values(torch, _ar, rows, c, nm.SEED, off)
    if not add:
        return xi, xi, None
    av = nm.ln_addvec(_ar, (rows + nm.ADDVEC_ROWS - 1) // nm.ADDVEC_ROWS + 1, c, nm.SEED)
    return xi, xi + av[_ar(rows) // nm.ADDVEC_ROWS], av


def _row_stats(xs):
    mean, rstd = exact_stats(xs.sum(1), (xs * xs).sum(1), xs.shape[1], nm.EPS_LN)
    ulp = torch.exp2(torch.floor(torch.log2(xs.abs().max(1).values.double().clamp_min(1.0))) - 23)
    return mean, rstd, ulp


def _ln_stats_launch(ops, sweep, tag, rows, c, off, add):
    """sp_ln_stats_f16 once: statistics within their bounds, sum_out bit for bit, the guard rows behind `rows` untouched"""
    xi, xs, av = _ln_inputs(rows, c, off, add)
    sbuf, stats = guarded(rows, 2, torch.float32)
    mbuf, sm = guarded(rows, c)
    kw = dict(addvec=av.half(), addvec_rows=nm.ADDVEC_ROWS, sum_out=sm) if add else {}
    ops.ln_stats(xi.half(), stats, rows=rows, c=c, eps=1e-5, **kw)
    mean, rstd, ulp = _row_stats(xs)
    sum_ok = ((sm.view(torch.int16) == xs.half().view(torch.int16)).all() if add else torch.isnan(sm).all()).reshape(1)
    sweep.add(tag, worst_ratio(stats[:, 0], mean, ulp), worst_ratio(stats[:, 1].double() / rstd, torch.ones_like(rstd),
                                                                     torch.full_like(rstd, 2.0 ** -18)),
              guards_intact(sbuf, rows), guards_intact(mbuf, rows), sum_ok)


@pytest.mark.parametrize("rows,c", nm.LN_WIDTHS)
def test_layernorm_counts_every_channel_once(rows, c):
    """sp_layernorm_f16 and sp_ln_stats_f16 (one wave per row): row r has its spike in channel r mod c and rows >= c, so every
    channel -- every octet lane + 64 i of every NV -- is the heavy one once; ragged row counts (rows % 4 != 0); with and
    without the per-frame pre-add, whose frame boundaries (50 rows) fall inside a block's four rows."""
    ops = _ops()
    p = nm.ln_plan(rows, c, False)
    assert p["kernel"] == "ln" and p["nv"] == min(4, (c // 8 + 63) // 64) and rows >= c and rows % 4 != 0
    assert nm.ln_plan(rows, c, True)["kernel"] == "ln_stats"
    gamma, beta = (t.double() for t in nm.affine(_ar, c))
    sweep, st_sweep = Sweep(f"layernorm {(rows, c)} ln<{p['nv']}>"), Sweep(f"ln_stats {(rows, c)} ln_stats<{p['nv']}>")
    for off in (0, 40):
        for add in (False, True):
            xi, xs, av = _ln_inputs(rows, c, off, add)
            buf, y = guarded(rows, c)
            mbuf, sm = guarded(rows, c)
            kw = dict(addvec=av.half(), addvec_rows=nm.ADDVEC_ROWS, sum_out=sm) if add else {}
            ops.layernorm(xi.half(), gamma.float(), beta.float(), y, rows=rows, c=c, eps=1e-5, **kw)
            mean, rstd, _ = _row_stats(xs)
            ref, bnd = reference(xs.double(), mean[:, None], rstd[:, None], gamma[None, :], beta[None, :], False, nm.sum_terms(p))
            sum_ok = ((sm.view(torch.int16) == xs.half().view(torch.int16)).all() if add else torch.isnan(sm).all()).reshape(1)
            sweep.add((off, add), worst_ratio(y, ref, bnd), guards_intact(buf, rows), guards_intact(mbuf, rows), sum_ok)
            _ln_stats_launch(ops, st_sweep, (off, add), rows, c, off, add)
    sweep.finish([c], ["y"], [1.0])
    st_sweep.finish([1, 1], ["mean", "rstd"], [1.0, 1.0])


@pytest.mark.parametrize("rows,c,kernel", [(8191, 320, "ln_stats"), (8192, 320, "ln_stats_rows"), (8193 + 5, 320, "ln_stats_rows"),
                                           (4097, 640, "ln_stats_rows"), (2049, 1280, "ln_stats_rows")])
def test_ln_stats_rows_per_wave_at_their_thresholds(rows, c, kernel):
    """sp_ln_stats_f16 around the row counts where the rows-per-wave kernels take over: ragged last waves (clamped rows are
    computed, not stored), with and without the pre-add and the written-out sum, a frame boundary inside a wave's rows"""
    ops = _ops()
    p = nm.ln_plan(rows, c, True)
    assert p["kernel"] == kernel and (rows, c) in nm.LN_ROWS_CASES
    if kernel == "ln_stats_rows":
        assert nm.ADDVEC_ROWS % p["rows_per_wave"] != 0 and (rows % p["rows_per_wave"] != 0 or rows == 8192)
    sweep = Sweep(f"ln_stats {(rows, c)} {kernel}")
    for off in (0, 40):
        for add in (False, True):
            _ln_stats_launch(ops, sweep, (off, add), rows, c, off, add)
    sweep.finish([1, 1], ["mean", "rstd"], [1.0, 1.0])
