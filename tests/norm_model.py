"""CPU model of csrc/norm.hip for the membership tests (tests/test_norm_membership_cpu.py, tests/test_norm_membership_gpu.py).

"Membership": every row and every channel of an (instance, group) slab -- or of a LayerNorm row -- enters the statistics
exactly once, and every element is written exactly once.  The suite's older yardstick (relative L2 <= 2e-3 on Gaussian
data) cannot tell that from "almost every row": one row of 9,216 moves the output by a twentieth of an fp16 ulp.

The spike design makes one row count.  Inputs are small integers in fp16 (base values -2, -1, 1, 2, optionally a per-group
offset of 0 / +-40), and every slab carries ONE spike row of amplitude A ~ sqrt(rows), so that row holds about as much of
the slab's sum of squares as all the other rows together: dropping or doubling it moves rstd by tens of percent, dropping
or doubling an ordinary row by ~1 / rows, which the per-element bound below still resolves at a few hundred rows.  The
spike MOVES: launch l puts slab s's spike on row (l * n_slabs + s) mod rows, so a sweep of ceil(rows / n_slabs) launches
makes every row the heavy one once, and a row a kernel forgets is caught on the launch that puts the spike there.

All sums of the design are integers far below 2^24, so fp32 accumulation is exact in ANY order and the kernels' statistics
are determined up to their final conversions; the reference statistics are exact integer sums divided in fp64.

This file holds: the data (one generator for numpy and for torch on a device), the exact statistics, the reference and
its per-element bound, the host's launch arithmetic restated (plan / tile_plan / ln_plan), fp32 restatements of every kernel
in its own order of operations, and the planted mistakes (MISTAKES) as variations of those restatements.  numpy only."""

import functools
import math

import numpy as np

EPS_GN = float(np.float32(1e-6))      # the kernels take eps as a float
EPS_LN = float(np.float32(1e-5))
U = 2.0 ** -24                        # half an fp32 ulp at 1
BOUND_K = 16.0                        # see reference()
HALF_TILE = 128                       # rows behind one record of a contraction's column sums
f32 = np.float32


# ------------------------------------------------------------------------------------------------ data
def amplitude(n):
    """the power of two nearest sqrt(n) (on the log scale)"""
    return 2 ** int(math.floor(0.5 * math.log2(n) + 0.5))


def _hash(idx, seed):
    """32-bit mix of an int64 index array / tensor (operators only: the same code runs under numpy and torch)"""
    t = (idx * 2654435761 + (seed * 40503 + 12345)) & 0xFFFFFFFF
    t = t ^ (t >> 15)
    t = (t * 0x45D9F3B) & 0xFFFFFFFF
    t = t ^ (t >> 13)
    return t


def _base(idx, seed):
    k = (_hash(idx, seed) >> 5) & 3
    return k - 2 + (k >> 1)           # -2, -1, 1, 2


def row_spike(launch, slab, n_slabs, rows):
    """the GroupNorm sweep: ceil(rows / n_slabs) launches put the spike on every row of every instance once"""
    return (launch * n_slabs + slab) % rows


def record_spike(launch, slab, n_slabs, rows):
    """the tile-sums sweep: rows / 128 launches put the spike into every half-tile record once (on varying rows of it)"""
    return ((launch + slab) % (rows // HALF_TILE)) * HALF_TILE + (5 * slab + 3 * launch) % HALF_TILE


def group_offsets(inst, g, offset):
    """-offset, 0, +offset by (instance + group) mod 3"""
    return offset * ((g + inst) % 3 - 1)


def spike_pattern(k, a):
    """+A on a group's even channels, -A/2 on its odd ones: two values, so that no single shift equals the row"""
    return a - (k & 1) * (a + a // 2)


def spike_values(xp, ar, instances, rows, c, groups, launch, seed, offset=0, spike_row=row_spike):
    """int64 [instances * rows][c]; xp = numpy or torch, ar(n) = that library's int64 arange(n)"""
    cpg = c // groups
    r = ar(instances * rows)[:, None]
    ch = ar(c)[None, :]
    base = _base(r * c + ch, seed)
    g = ch // cpg
    k = ch - g * cpg
    inst = r // rows
    rr = r - inst * rows
    srow = spike_row(launch, inst * groups + g, instances * groups, rows)
    # the slab's first element stays a base value: it is gn_stats_kernel's shift reference
    is_spike = (rr == srow) & ~((rr == 0) & (k == 0))
    return xp.where(is_spike, spike_pattern(k, amplitude(rows)), base) + group_offsets(inst, g, offset)


def _ar(n):
    return np.arange(n, dtype=np.int64)


def spike_slabs(instances, rows, c, groups, launch, seed, offset=0, spike_row=row_spike):
    """integer-valued fp16 input [instances * rows][c]"""
    return spike_values(np, _ar, instances, rows, c, groups, launch, seed, offset, spike_row).astype(np.float16)


def affine(ar, c):
    """gamma / beta per channel: exact in fp32, different in neighbouring octets, gamma of both signs"""
    ch = ar(c)
    gamma = (0.5 + ((ch * 37) % 64) / 64.0) * (1 - 2 * ((ch % 5) == 0))
    beta = ((ch * 53) % 97 - 48) / 32.0
    return gamma, beta


def ln_values(xp, ar, rows, c, seed, offset=0):
    """LayerNorm input, int64 [rows][c]: row r has its spike in channel r mod c (+A on even rows, -A/2 on odd ones, A the power
    of two nearest sqrt(c)), and an offset of -offset / 0 / +offset by row"""
    r = ar(rows)[:, None]
    ch = ar(c)[None, :]
    base = _base(r * c + ch, seed)
    return xp.where(ch == r % c, spike_pattern(r, amplitude(c)), base) + offset * (r % 3 - 1)


def ln_addvec(ar, frames, c, seed):
    """the per-frame vector that is added in front of the LayerNorm, int64 [frames][c], values -6 .. 6"""
    f = ar(frames)[:, None]
    ch = ar(c)[None, :]
    return 3 * _base(f * c + ch, seed + 77)


# ------------------------------------------------------------------------------------------------ exact statistics
def _exact(s1, s2, n, eps):
    mean = s1 / float(n)
    var = (n * s2 - s1 * s1) / float(n) / float(n)        # the numerator is an exact integer
    return mean, var, 1.0 / np.sqrt(var + eps)


def slab_stats(x, instances, rows, c, groups, eps=EPS_GN):
    """exact (mean, var, rstd) per (instance, group) in fp64 from integer sums; x: integer-valued [instances * rows][c]"""
    cpg = c // groups
    xi = np.asarray(x).astype(np.int64).reshape(instances, rows, groups, cpg)
    return _exact(xi.sum(axis=(1, 3)), (xi * xi).sum(axis=(1, 3)), rows * cpg, eps)


def row_stats(x, eps=EPS_LN):
    xi = np.asarray(x).astype(np.int64)
    return _exact(xi.sum(1), (xi * xi).sum(1), xi.shape[1], eps)


# ------------------------------------------------------------------------------------------------ reference and bound
def ulp16(v):
    """one fp16 ulp at |v| (2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(e - 10)


def silu64(v):
    return v / (1.0 + np.exp(-v))


def reference(x, mean, rstd, gamma, beta, silu, sum_terms=0):
    """y = (x - mean) * rstd * gamma + beta in fp64 (+ SiLU), and the bound per element.

    bound = one fp16 ulp of the reference + 16 * 2^-24 * (|x sc| + |mean sc| + |beta|), sc = rstd * gamma.  A correctly
    rounded fp16 store is half an ulp; the fp32 part counts, in units of 2^-24 of the larger operand, the rounding of sc,
    of sf = beta - mean * sc, of the multiply-add, the two statistics conversions (mean, rstd to fp32), and silu_f's
    hardware exp2 and rcp (one ulp each, i.e. two units) -- eight units, doubled.  With SiLU the fp32 term passes through
    the derivative, which is at most 1.1.

    sum_terms: where a kernel adds squared DEVIATIONS in fp32 (gn_fused_kernel: MAXIT * VEC per thread and six butterfly adds;
    ln_kernel: 8 NV and six) the sum is not one of integers and every add rounds: the variance is off by at most
    sum_terms * 2^-24 relative, rstd by half of that, and, doubled like the rest, the bound grows by
    sum_terms * 2^-24 * |(x - mean) sc|.  (The shifted sums of gn_stats_kernel and the tile sums are integers: 0 there.)
    The fused restatement first showed this: 0.5000003 of the bound without the term, rstd eight units off."""
    sc = rstd * gamma
    pre = (x - mean) * sc + beta
    slack = BOUND_K * U * (np.abs(x * sc) + np.abs(mean * sc) + np.abs(beta)) + sum_terms * U * np.abs((x - mean) * sc)
    if silu:
        ref = silu64(pre)
        return ref, ulp16(ref) + 1.1 * slack
    return pre, ulp16(pre) + slack


# ------------------------------------------------------------------------------------------------ launch plans
def _rows_per_iter(oc):
    return max(1, 512 // oc)


def _round_up(a, b):
    return (a + b - 1) // b * b


def apply_partition(instances, rows, P):
    blocks_y = (2048 + instances - 1) // instances
    blocks_y = max(1, min(blocks_y, (rows + 16 * P - 1) // (16 * P)))
    rpb = _round_up((rows + blocks_y - 1) // blocks_y, 4 * P)
    return rpb, (rows + rpb - 1) // rpb


def plan(instances, rows, c, groups):
    """sp_groupnorm_ld_f16's host arithmetic: which kernels run, and how they cut the rows"""
    cpg = c // groups
    oc = c // 8
    P = _rows_per_iter(oc)
    p = dict(route="split", cpg=cpg, oc=oc, P=P, threads=max(64, _round_up(oc * P, 64)))
    if cpg % 8 == 0 and cpg // 8 <= 512 and (instances * groups >= 128 or instances * rows * c * 2 <= (8 << 20)):
        vpr = cpg // 8
        rp = 512 // vpr
        for maxit in (16, 20):
            if rows <= maxit * rp:
                p.update(route="fused", vpr=vpr, rp=rp, maxit=maxit, idle=512 - rp * vpr)
                return p
    want = (1024 + instances - 1) // instances
    want = max(1, min(want, max(1, rows // (16 * P)), 512))
    per = _round_up((rows + want - 1) // want, 4 * P)
    splits = (rows + per - 1) // per
    rpb, blocks_y = apply_partition(instances, rows, P)
    p.update(per=per, splits=splits, fold_in_apply=splits <= 128, rpb=rpb, blocks_y=blocks_y)
    return p


def sum_terms(p):
    """fp32 adds of squared deviations behind one variance (see reference()); p: a plan() or ln_plan() record"""
    if p.get("route") == "fused":
        return p["maxit"] * 8 + 6
    if p.get("kernel") in ("ln", "ln_stats"):
        return p["nv"] * 8 + 6
    if p.get("kernel") == "ln_stats_rows":
        return 40 + 6
    return 0


def tile_plan(instances, rows, c, groups):
    """sp_groupnorm_tile_sums2_f16: one finalize block per (instance, group) over 2 * rows / 256 records, then the apply pass"""
    assert rows % 256 == 0
    P = _rows_per_iter(c // 8)
    rpb, blocks_y = apply_partition(instances, rows, P)
    return dict(route="tile_sums", cpg=c // groups, P=P, records=rows // HALF_TILE, rpb=rpb, blocks_y=blocks_y)


def ln_plan(rows, c, stats_only):
    oc = c // 8
    if stats_only:
        for cc, lpr, thr in ((320, 8, 8192), (640, 16, 4096), (1280, 32, 2048)):
            if c == cc and rows >= thr:
                return dict(kernel="ln_stats_rows", lpr=lpr, passes=2, rows_per_wave=2 * (64 // lpr))
    return dict(kernel="ln_stats" if stats_only else "ln", nv=min(4, (oc + 63) // 64), oc=oc, rows_per_wave=1)


# ------------------------------------------------------------------------------------------------ walks (membership)
@functools.lru_cache(maxsize=None)
def row_walk(rows, P, per, blocks, *, skip_tail=(), double_first=False, clamp=True):
    """How often gn_stats_kernel / gn_apply_kernel touch each instance-relative row: `blocks` blocks of `per` rows, every
    block's P row-threads in double-buffered batches of four rows P apart, then the scalar tail loop.  Returns the
    multiplicity of rows 0 .. blocks * per (rows behind `rows` belong to the next instance).  skip_tail: blocks whose tail
    loop is left out; double_first: the first row of every block taken twice; clamp=False: r1 not cut at `rows`."""
    m = np.zeros(blocks * per + 4 * P, dtype=np.int64)
    step = 4 * P
    for b in range(blocks):
        r0 = b * per
        r1 = r0 + per
        if clamp and r1 > rows:
            r1 = rows
        for pr in range(P):
            r = r0 + pr
            if r + 3 * P < r1:
                while True:
                    for u in range(4):
                        m[r + u * P] += 1
                    r += step
                    if not r + 3 * P < r1:
                        break
            while r < r1:
                if b not in skip_tail:
                    m[r] += 1
                r += P
        if double_first:
            m[r0] += 1
    return m


def fused_walk(rows, vpr, maxit, *, idle_live=False, drop_last=False):
    """gn_fused_kernel: thread t holds vector t % vpr of row t / vpr + it * rp in pass it.  Returns (row [maxit][512],
    vector [512], live [maxit][512])."""
    rp = 512 // vpr
    tid = np.arange(512)
    q, rr = tid % vpr, tid // vpr
    row = rr[None, :] + np.arange(maxit)[:, None] * rp
    live = (row < rows) & ((rr < rp) | idle_live)[None, :]
    if drop_last:
        live[maxit - 1] = False
    return row, q, live


# ------------------------------------------------------------------------------------------------ fp32 helpers
def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def _silu_f(v):
    """v * rcp(1 + exp2(-log2(e) * v)) in fp32"""
    with np.errstate(over="ignore"):
        t = np.exp2((f32(-1.4426950408889634) * v).astype(f32).astype(np.float64)).astype(f32)
    return (v * (f32(1.0) / (f32(1.0) + t)).astype(f32)).astype(f32)


def _butterfly(v, width=64):
    """v += shfl_xor(v, o) for o = width / 2 .. 1 over the last axis (lanes), in fp32"""
    lane = np.arange(v.shape[-1])
    o = width // 2
    while o > 0:
        v = (v + v[..., lane ^ o]).astype(f32)
        o >>= 1
    return v


def apply_f32(x, mean32, rstd32, gamma, beta, silu):
    """gn_apply_kernel / gn_fused_kernel's arithmetic in fp32: sc = rstd * gamma, sf = beta - mean * sc, y = x * sc + sf"""
    sc = (rstd32.astype(f32) * gamma.astype(f32)).astype(f32)
    sf = _fma(-mean32.astype(f32), sc, beta.astype(f32))
    y = _fma(x.astype(f32), sc, sf)
    if silu:
        y = _silu_f(y)
    return y.astype(np.float16)


# ------------------------------------------------------------------------------------------------ GroupNorm restatements
class Case:
    """What all launches of one (instances, rows, c, groups, seed) share: the base values and their per-row sums."""

    def __init__(self, instances, rows, c, groups, seed):
        self.instances, self.rows, self.c, self.groups, self.seed = instances, rows, c, groups, seed
        self.cpg = c // groups
        R = instances * rows
        self.base = _base(_ar(R)[:, None] * c + _ar(c)[None, :], seed).astype(np.int8)          # [R][c]
        b = self.base.reshape(R, groups, self.cpg).astype(np.int64)
        self.b1, self.b2 = b.sum(2), (b * b).sum(2)                                             # [R][groups]
        self.first = b[:, :, 0].copy()
        bi = self.base.reshape(instances, rows, c)
        self.wbase = np.stack([(bi == v).sum(1) for v in (-2, -1, 1, 2)], axis=-1)               # [inst][c][4]
        self.gamma, self.beta = affine(_ar, c)
        self._pb = None

    def part_base(self):
        if self._pb is None:
            b = self.base.reshape(-1, HALF_TILE, self.c).astype(np.int64)
            self._pb = (b.sum(1), (b * b).sum(1))                                               # [records][c]
        return self._pb


class Slabs:
    """One launch of the spike design, kept as per-row, per-group integer sums (and x itself only where asked for)."""

    def __init__(self, case, launch, offset=0, spike_row=row_spike):
        cs = self.case = case
        self.instances, self.rows, self.c, self.groups, self.cpg = cs.instances, cs.rows, cs.c, cs.groups, cs.cpg
        self.launch, self.offset = launch, offset
        inst, g = np.meshgrid(_ar(cs.instances), _ar(cs.groups), indexing="ij")
        self.off = group_offsets(inst, g, offset)                                               # [inst][groups]
        self.srow = spike_row(launch, inst * cs.groups + g, cs.instances * cs.groups, cs.rows)
        self.gamma, self.beta = cs.gamma, cs.beta
        k = _ar(cs.cpg)
        # the spike rows themselves: [inst][groups][cpg]
        grow = inst * cs.rows + self.srow
        brow = cs.base.reshape(-1, cs.groups, cs.cpg)[grow, g].astype(np.int64)
        keep = (self.srow == 0)[:, :, None] & (k == 0)[None, None, :]
        self.spike_vals = np.where(keep, brow, spike_pattern(k, amplitude(cs.rows))[None, None, :]) + self.off[:, :, None]
        offr = np.repeat(self.off, cs.rows, axis=0)                                             # [R][groups]
        self.x1 = cs.b1 + cs.cpg * offr
        self.x2 = cs.b2 + 2 * offr * cs.b1 + cs.cpg * offr * offr
        self.xf = cs.first + offr                                                               # the group's first channel
        self.x1[grow, g] = self.spike_vals.sum(2)
        self.x2[grow, g] = (self.spike_vals * self.spike_vals).sum(2)
        self.xf[grow, g] = self.spike_vals[:, :, 0]
        n = cs.rows * cs.cpg
        self.mean, self.var, self.rstd = _exact(self.x1.reshape(cs.instances, cs.rows, cs.groups).sum(1),
                                                self.x2.reshape(cs.instances, cs.rows, cs.groups).sum(1), n, EPS_GN)

    @property
    def x(self):
        """int64 [instances * rows][c]"""
        cs = self.case
        x = cs.base.reshape(cs.instances, cs.rows, cs.groups, cs.cpg).astype(np.int64) + self.off[:, None, :, None]
        inst, g = np.meshgrid(_ar(cs.instances), _ar(cs.groups), indexing="ij")
        x[inst, self.srow, g] = self.spike_vals
        return x.reshape(cs.instances * cs.rows, cs.c)

    def part(self):
        """the contraction's half-tile column sums of this launch, fp32 [records][c][2] (exact integers)"""
        cs = self.case
        p1, p2 = cs.part_base()
        recs = cs.rows // HALF_TILE
        offc = np.repeat(np.repeat(self.off, cs.cpg, axis=1), recs, axis=0)                     # [records][c]
        s1 = p1 + HALF_TILE * offc
        s2 = p2 + 2 * offc * p1 + HALF_TILE * offc * offc
        inst, g = np.meshgrid(_ar(cs.instances), _ar(cs.groups), indexing="ij")
        grow = inst * cs.rows + self.srow
        old = cs.base.reshape(-1, cs.groups, cs.cpg)[grow, g].astype(np.int64) + self.off[:, :, None]
        rec = (grow // HALF_TILE)[:, :, None]
        ch = (g * cs.cpg)[:, :, None] + _ar(cs.cpg)[None, None, :]
        np.add.at(s1, (rec, ch), self.spike_vals - old)
        np.add.at(s2, (rec, ch), self.spike_vals * self.spike_vals - old * old)
        assert max(np.abs(s1).max(), s2.max()) < 2 ** 24
        return np.stack([s1, s2], axis=-1).astype(f32)

    def value_table(self):
        """Every distinct (value, channel) pair of each instance and how many rows carry it (y depends on nothing else):
        values [inst][c][6] -- four base values, +A, -A/2 -- and weights [inst][c][6].  The base weights are those of the
        case without its spike rows (off by one at most)."""
        cs = self.case
        a = amplitude(cs.rows)
        offc = np.repeat(self.off, cs.cpg, axis=1)                                              # [inst][c]
        cand = np.array([-2, -1, 1, 2, a, -(a // 2)])[None, None, :] + offc[:, :, None]
        sv = self.spike_vals.reshape(cs.instances, cs.c)
        w = np.concatenate([cs.wbase, (sv == cand[:, :, 4])[:, :, None], (sv == cand[:, :, 5])[:, :, None]], axis=-1)
        return cand, w

    def worst(self, mean32, rstd32, silu, gamma_idx=None, unwritten=False, sum_terms=0):
        """The largest |y - ref| / bound over all elements when the kernel applies (mean32, rstd32) [inst][groups] in fp32,
        and what tests/test_kernels_gpu.py's check() measures on the same output (relative L2, max error / max|ref|)."""
        cand, w = self.value_table()
        g = np.arange(self.c) // self.cpg
        ga, be = self.gamma, self.beta
        gi = np.arange(self.c) if gamma_idx is None else gamma_idx
        ref, bnd = reference(cand.astype(np.float64), self.mean[:, g, None], self.rstd[:, g, None], ga[None, :, None],
                             be[None, :, None], silu, sum_terms)
        y = apply_f32(cand, mean32[:, g, None], rstd32[:, g, None], ga[gi][None, :, None], be[gi][None, :, None], silu)
        err = np.where(w > 0, np.abs(y.astype(np.float64) - ref), 0.0)
        l2 = math.sqrt(float((w * err * err).sum()) / float((w * ref * ref).sum()))
        mx = float(err.max() / np.where(w > 0, np.abs(ref), 0.0).max())
        return dict(factor=math.inf if unwritten else float((err / bnd).max()), rel_l2=l2, max_rel=mx)


def gn_split_stats(s, p, mistake=None):
    """gn_stats_kernel + the fp64 fold (gn_finalize_kernel, or gn_apply_kernel's prologue: the same arithmetic): shifted sums
    over the rows the walk visits, exact in fp32 because they are integers below 2^24; -> (mean, rstd) fp32 [inst][groups]"""
    inst, rows, groups, cpg = s.instances, s.rows, s.groups, s.cpg
    m = row_walk(rows, p["P"], p["per"], p["splits"], skip_tail=tuple(range(p["splits"])) if mistake == "stats_tail_skipped" else (),
                 double_first=mistake == "stats_first_row_twice", clamp=mistake != "stats_r1_not_clamped")
    pad = np.zeros((len(m), groups), dtype=np.int64)                        # behind the tensor: nothing
    x1, x2, xf = (np.concatenate([t, pad]) for t in (s.x1, s.x2, s.xf))
    ref = s.xf.reshape(inst, rows, groups)[:, 0]                            # the group's first element of the first row
    mean32 = np.zeros((inst, groups), dtype=f32)
    rstd32 = np.zeros((inst, groups), dtype=f32)
    cnt = float((p["splits"] * p["per"] if mistake == "stats_count_padded" else rows) * cpg)
    for i in range(inst):
        sl = slice(i * rows, i * rows + len(m))                             # behind `rows`: the next instance
        r = ref[i][None, :]
        d1 = x1[sl] - cpg * r
        d2 = x2[sl] - 2 * r * x1[sl] + cpg * r * r
        if mistake == "group_boundary_channel":
            # the fold of group g takes channels g * cpg + 1 .. (g + 1) * cpg: its first channel is lost, the neighbour's
            # first channel (shifted by the neighbour's reference) comes in; the last group reads nothing there
            df = xf[sl] - r
            dn = np.concatenate([df[:, 1:], np.zeros_like(df[:, :1])], axis=1)
            d1 = d1 - df + dn
            d2 = d2 - df * df + dn * dn
        a = (m[:, None] * d1).sum(0)
        b = (m[:, None] * d2).sum(0)
        assert np.abs(a).max() < 2 ** 24 and b.max() < 2 ** 24, "the design's sums must stay exact in fp32"
        dmean = a.astype(f32).astype(np.float64) / cnt
        var = np.maximum(b.astype(f32).astype(np.float64) / cnt - dmean * dmean, 0.0)
        mean32[i] = (ref[i].astype(np.float64) + dmean).astype(f32)
        rstd32[i] = (1.0 / np.sqrt(var + EPS_GN)).astype(f32)
    return mean32, rstd32


def _apply_route(s, p, mean32, rstd32, silu, mistake):
    gamma_idx = (np.arange(s.c) + 8) % s.c if mistake == "gamma_beta_neighbour_octet" else None
    last = p["blocks_y"] - 1
    m = row_walk(s.rows, p["P"], p["rpb"], p["blocks_y"], skip_tail=(last,) if mistake == "apply_tail_rows_left" else ())
    assert m[s.rows:].sum() == 0
    assert mistake == "apply_tail_rows_left" or (m[:s.rows] == 1).all(), "the apply walk must write every row once"
    return s.worst(mean32, rstd32, silu, gamma_idx, unwritten=bool((m[:s.rows] == 0).any()))


def gn_split(s, silu, mistake=None):
    p = plan(s.instances, s.rows, s.c, s.groups)
    assert p["route"] == "split"
    mean32, rstd32 = gn_split_stats(s, p, mistake)
    return _apply_route(s, p, mean32, rstd32, silu, mistake)


def gn_fused_stats(s, p, mistake=None):
    """gn_fused_kernel: the integer sum -> fp32 mean; then per thread the fp32 sum of its live MAXIT * VEC squared deviations,
    a wave butterfly, and eight wave partials folded in fp64.  Returns (mean, rstd) fp32 [inst][groups] and how many
    threads hold each row."""
    inst, rows, groups, cpg = s.instances, s.rows, s.groups, s.cpg
    vpr, maxit = p["vpr"], p["maxit"]
    row, q, live = fused_walk(rows, vpr, maxit, idle_live=mistake == "fused_idle_threads_live",
                              drop_last=mistake == "fused_last_pass_missing")
    x5 = np.zeros((int(row.max()) + 1, vpr, inst, groups, 8), dtype=np.int64)
    x5[:rows] = np.moveaxis(s.x.reshape(inst, rows, groups, vpr, 8), (1, 3), (0, 1))
    v = np.where(live[:, :, None, None, None], x5[row, q[None, :]], 0)      # [maxit][512][inst][groups][8]
    cnt = float(rows * cpg)
    s1 = v.sum(axis=(0, 1, 4))
    assert np.abs(s1).max() < 2 ** 24
    mean32 = (s1.astype(np.float64) / cnt).astype(f32)                      # [inst][groups]
    ss = np.zeros((512, inst, groups), dtype=f32)
    for it in range(maxit):
        for e in range(8):
            d = (v[it, :, :, :, e].astype(f32) - mean32[None]).astype(f32)
            ss = np.where(live[it][:, None, None], _fma(d, d, ss), ss)
    waves = _butterfly(np.moveaxis(ss, 0, -1).reshape(inst, groups, 8, 64))[..., 0].astype(np.float64)
    b = np.zeros((inst, groups))
    for w in range(8):
        b = b + waves[..., w]
    rstd32 = (1.0 / np.sqrt(b / cnt + EPS_GN)).astype(f32)
    held = np.zeros(int(row.max()) + 1, dtype=np.int64)
    np.add.at(held, row[live], 1)
    return mean32, rstd32, held[:rows]


def gn_fused(s, silu, mistake=None):
    p = plan(s.instances, s.rows, s.c, s.groups)
    assert p["route"] == "fused"
    mean32, rstd32, held = gn_fused_stats(s, p, mistake)
    assert mistake is not None or (held == p["vpr"]).all(), "every vector of every row is held by one thread"
    gamma_idx = (np.arange(s.c) + 8) % s.c if mistake == "gamma_beta_neighbour_octet" else None
    return s.worst(mean32, rstd32, silu, gamma_idx, unwritten=bool((held == 0).any()), sum_terms=sum_terms(p))


def gn(s, silu, mistake=None):
    return (gn_fused if plan(s.instances, s.rows, s.c, s.groups)["route"] == "fused" else gn_split)(s, silu, mistake)


# ------------------------------------------------------------------------------------------------ tile-sums restatement
def gn_tile_sums_stats(part, instances, rows, c, groups, part_b=None, c_a=None, mistake=None):
    """gn_tile_sums_finalize_kernel: thread t folds records t, t + 256, ... (fp32 over a record's cpg pairs, fp64 across
    records), thread 0 folds the thread partials in fp64; un-shifted sums.  part: fp32 [records][c or c_a][2], part_b:
    fp32 [records][c - c_a][2].  -> stats fp32 [inst][groups][2]"""
    cpg = c // groups
    recs = rows // HALF_TILE
    flat_a = np.concatenate([part.reshape(-1, 2), np.zeros((c, 2), dtype=f32)])                 # (behind the buffer: nothing)
    flat_b = part_b.reshape(-1, 2) if part_b is not None else None
    r = (_ar(instances)[:, None, None] * recs + _ar(recs)[None, None, :])                       # [inst][1][records]
    sa = np.zeros((instances, groups, recs, 2), dtype=f32)
    for k in range(cpg):
        ch = (_ar(groups) * cpg + k)[None, :, None]
        if part_b is None:
            v = flat_a[r * c + ch]
        else:
            pitch = c_a if mistake == "tile_seam_pitch" else c - c_a
            # the producer is chosen per CHANNEL: a group that straddles the seam takes some channels from each.  The planted
            # mistake chooses it once per group, from the group's first channel, and walks on in that producer's record
            first = ch - k if mistake == "tile_producer_per_group" else ch
            ia = np.where(first < c_a, r * c_a + ch, 0)
            ib = np.where(first < c_a, 0, r * pitch + (ch - c_a))
            v = np.where((first < c_a)[..., None], flat_a[ia], flat_b[ib])
        sa = (sa + v).astype(f32)
    if mistake == "tile_fold_stops_at_256":
        sa = sa[:, :, :256]
    ab = sa.astype(np.float64).sum(2)                                                           # integers: any order
    cnt = float(rows * cpg)
    mean = ab[..., 0] / cnt
    var = np.maximum(ab[..., 1] / cnt - mean * mean, 0.0)
    return np.stack([mean.astype(f32), (1.0 / np.sqrt(var + EPS_GN)).astype(f32)], axis=-1)


def gn_tile_sums(s, silu, c_a=None, mistake=None):
    part = s.part()
    pa, pb = part, None
    if c_a is not None:
        pa, pb = np.ascontiguousarray(part[:, :c_a]), np.ascontiguousarray(part[:, c_a:])
    stats = gn_tile_sums_stats(pa, s.instances, s.rows, s.c, s.groups, pb, c_a, mistake)
    p = tile_plan(s.instances, s.rows, s.c, s.groups)
    out = _apply_route(s, p, stats[..., 0], stats[..., 1], silu, mistake)
    out["stats"] = stats
    return out


def tile_stats_bounds(mean):
    """the returned statistics: the mean within one fp32 ulp of its own binade (a mean of exactly 0 must come back as 0),
    rstd within 2^-22 relative (one conversion of an fp64 value, with room for the fp64 cancellation of E[x^2] - mean^2 at a
    40-sigma offset)"""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(mean), 2.0 ** -126))) - 23), 2.0 ** -22


def fold_linear_reference(w, gamma, beta, bias, mean, rstd, cpg, w_out_got):
    """sp_groupnorm_fold_linear*: w_out = w * gamma * rstd[group] rounded to fp16 (bound: one fp16 ulp of the fp64 value), and
    bias_out = sum_c (beta w - mean * w_out) + bias with w_out the ROUNDED weights the kernel stored, so that a group's
    constant offset cancels exactly in the contraction.  bias bound: every lane adds 16 * ceil(oc / 64) products in fp32, the
    wave butterfly six more, the bias one, each product and the fp32 mean one rounding: (2 * 16 * ceil(oc / 64) + 8) units
    of 2^-24 of sum(|beta w| + |mean w_out|) + |bias|.  All arrays fp64; mean / rstd [inst][groups]."""
    c = w.shape[1]
    g = np.arange(c) // cpg
    w_ref = w[None] * (gamma[None, :] * rstd[:, g])[:, None, :]
    b_ref = (beta[None, None, :] * w[None] - mean[:, g][:, None, :] * w_out_got).sum(-1) + bias[None, :]
    mag = (np.abs(beta[None, None, :] * w[None]) + np.abs(mean[:, g][:, None, :] * w_out_got)).sum(-1) + np.abs(bias)[None, :]
    return w_ref, ulp16(w_ref), b_ref, fold_bias_units(c) * U * mag


def fold_bias_units(c):
    return 2 * 16 * ((c // 8 + 63) // 64) + 8


# ------------------------------------------------------------------------------------------------ LayerNorm restatements
class Rows:
    def __init__(self, rows, c, seed, offset=0, addvec_rows=0):
        self.rows, self.c = rows, c
        self.x = ln_values(np, _ar, rows, c, seed, offset)
        self.addvec_rows = addvec_rows
        self.add = None
        if addvec_rows:
            self.add = ln_addvec(_ar, (rows + addvec_rows - 1) // addvec_rows + 1, c, seed)
        self.gamma, self.beta = affine(_ar, c)

    def summed(self, shift=0):
        """x + addvec[(row + shift) / addvec_rows] -- integers, exact in fp16"""
        if self.add is None:
            return self.x
        return self.x + self.add[(np.arange(self.rows) + shift) // self.addvec_rows]


def ln_wave_per_row(r, mistake=None):
    """ln_kernel / ln_stats_kernel<NV>: lane l holds octets l + 64 i; integer sum -> mean = S / c in fp32; the lane's fp32 sum
    of squared deviations in (i, e) order, a 64-lane butterfly, rstd = rsqrt(ss / c + eps).  -> xs, mean32, rstd32 [rows]"""
    rows, c = r.rows, r.c
    oc = c // 8
    nv = min(4, (oc + 63) // 64)
    xs = r.summed(1 if mistake == "ln_addvec_row_plus_one" else 0)
    v = np.zeros((rows, nv * 64, 8), dtype=np.int64)
    v[:, :oc] = xs.reshape(rows, oc, 8)
    v = v.reshape(rows, nv, 64, 8)
    have = (np.arange(nv)[:, None] * 64 + np.arange(64)[None, :]) < oc          # [nv][64]
    if mistake == "ln_octets_beyond_64_missing":
        have = have & (np.arange(nv)[:, None] < 1)
        v = np.where(have[None, :, :, None], v, 0)
    s1 = v.sum(axis=(1, 2, 3))
    assert np.abs(s1).max() < 2 ** 24
    mean32 = (s1.astype(f32) / f32(c)).astype(f32)
    ss = np.zeros((rows, 64), dtype=f32)
    for i in range(nv):
        for e in range(8):
            d = (v[:, i, :, e].astype(f32) - mean32[:, None]).astype(f32)
            ss = np.where(have[i][None, :], _fma(d, d, ss), ss)
    tot = _butterfly(ss)[:, 0]
    rstd32 = (f32(1.0) / np.sqrt(((tot / f32(c)).astype(f32) + f32(EPS_LN)).astype(f32))).astype(f32)
    return xs, mean32, rstd32


def ln_rows_per_wave(r, lpr, mistake=None):
    """ln_stats_rows_kernel<LPR, 2>: LPR lanes share a row, lane li holds octets j * LPR + li (j < 5); the mean is the integer
    sum TIMES the fp32 reciprocal of C; squared deviations per lane in (j, e) order, a butterfly over LPR lanes,
    rstd = rsqrt(ss * (1 / C) + eps).  -> xs, mean32, rstd32 [rows], and the number of rows the kernel stores.
    (A clamped ragged row holds row rows - 1's own data, so stored over row rows - 1 it would change nothing; the form of
    that mistake that can be seen is the missing store guard, which writes behind `rows`.)"""
    rows, c = r.rows, r.c
    assert c == 40 * lpr
    xs = r.summed(1 if mistake == "ln_addvec_row_plus_one" else 0)
    v = xs.reshape(rows, 5, lpr, 8)                                            # octet = j * LPR + li
    s1 = v.sum(axis=(1, 2, 3))
    inv = f32(1.0) / f32(c)
    mean32 = (s1.astype(f32) * inv).astype(f32)
    ss = np.zeros((rows, lpr), dtype=f32)
    for j in range(5):
        for e in range(8):
            d = (v[:, j, :, e].astype(f32) - mean32[:, None]).astype(f32)
            ss = _fma(d, d, ss)
    tot = _butterfly(ss, lpr)[:, 0]
    rstd32 = (f32(1.0) / np.sqrt(_fma(tot, inv, f32(EPS_LN)))).astype(f32)
    stored = _round_up(rows, 2 * (64 // lpr)) if mistake == "ln_rows_clamped_row_stored" else rows
    return xs, mean32, rstd32, stored


def ln_stats_bounds(xs):
    """what the statistics are held to: the mean within one fp32 ulp of max|x| (the integer sum is exact; the division, or the
    multiplication by the rounded 1 / C, is within an ulp of the quotient, which is at most max|x|), rstd within 2^-18
    relative: at most 40 fp32 squares per lane, each carrying the mean's rounding, six butterfly adds and the rsqrt."""
    mx = np.abs(xs).max(1).astype(np.float64)
    return 2.0 ** (np.floor(np.log2(np.maximum(mx, 1.0))) - 23), 2.0 ** -18


def ln_apply(xs, mean32, rstd32, gamma, beta):
    """ln_kernel's output: ((v - mean) * rstd) * gamma + beta in fp32, rounded to fp16"""
    t = (xs.astype(f32) - mean32[:, None]).astype(f32)
    t = (t * rstd32[:, None]).astype(f32)
    return _fma(t, gamma.astype(f32)[None, :], beta.astype(f32)[None, :]).astype(np.float16)


def ln_check(r, xs, mean32, rstd32, with_y, stored=None):
    """worst ratios of a LayerNorm restatement against the exact statistics of the TRUE summed input: mean error / one ulp,
    rstd relative error / 2^-18, y error / bound; whether sum_out is the true sum and the guard row is left alone"""
    xt = r.summed()
    mean, var, rstd = row_stats(xt)
    ulp, rel = ln_stats_bounds(xt)
    out = dict(mean=float((np.abs(mean32.astype(np.float64) - mean) / ulp).max()),
               rstd=float((np.abs(rstd32.astype(np.float64) / rstd - 1.0) / rel).max()),
               sum_equal=bool((xs == xt).all()), guard_ok=stored is None or stored <= r.rows, y=0.0)
    if with_y:
        ref, bnd = reference(xt.astype(np.float64), mean[:, None], rstd[:, None], r.gamma[None, :], r.beta[None, :], False,
                             sum_terms(ln_plan(r.rows, r.c, False)))
        y = ln_apply(xs, mean32, rstd32, r.gamma, r.beta)
        out["y"] = float((np.abs(y.astype(np.float64) - ref) / bnd).max())
    return out


# ------------------------------------------------------------------------------------------------ cases and mistakes
GROUPS = 32
SEED = 5
# (instances, rows, c): what each case is there for is asserted from plan() in the tests
GN_SPLIT_CASES = [(2, 300, 320), (2, 1000, 320), (3, 1000, 640), (1, 4099, 2560), (1, 2041, 1280), (2, 1020, 2560),
                  (1, 9219, 64)]
# Several thousand rows, where the older check() really is blind: eight splits of 1,280 rows, the last of 259 (one batch of
# 4 P = 256 and a tail of three rows).  "First row of a split twice" is 8 rows of 9,219, "tail skipped" is 3.
LARGE_CASE = (1, 9219, 64)
LARGE_MISTAKES = ("stats_first_row_twice", "stats_tail_skipped")
GN_FUSED_CASES = [(4, 200, 256), (1, 8192, 256), (1, 1632, 1280), (1, 1633, 1280), (1, 2040, 1280), (1, 1020, 2560)]
# (instances, rows, c, c_a).  With 64 channels in 32 groups a group is two channels and the host wants c_a % 4 == 0, so the
# seam at 24 falls BETWEEN groups 11 and 12: groups on either side read one producer each.  With 256 channels a group is
# eight, and the seam at 20 falls INSIDE group 2 (channels 16 .. 23: four from each producer), as a 1,280 + 640 concatenation
# in 60-channel groups does.
TILE_CASES = [(2, 512, 64, None), (1, 33280, 64, None), (2, 512, 64, 24), (2, 512, 256, 20)]
LN_WIDTHS = [(65, 64), (322, 320), (523, 520), (641, 640), (1034, 1032), (1283, 1280), (1545, 1544), (2050, 2048)]
LN_ROWS_CASES = [(8191, 320), (8192, 320), (8193 + 5, 320), (4097, 640), (2049, 1280)]
ADDVEC_ROWS = 50
COMBOS = [(0, 0), (1, 0), (0, 40), (1, 40)]                                        # (silu, offset)


def launches(instances, rows, groups=GROUPS):
    return -(-rows // (instances * groups))


# name -> (route whose GPU sweep shows it, the case of that sweep the CPU test runs it on, kind)
# kind "statistics": one row / channel / record of a slab's statistics is wrong -- what the older check() cannot see;
# kind "placement": rows left unwritten or a vector taken from the neighbour -- visible to any elementwise check on random
# data, listed so that the per-element test is known to cover them as well.
MISTAKES = {
    "stats_tail_skipped": ("split", (2, 1000, 320), "statistics"),
    "stats_first_row_twice": ("split", (2, 300, 320), "statistics"),
    "stats_r1_not_clamped": ("split", (2, 1000, 320), "statistics"),
    "stats_count_padded": ("split", (2, 1000, 320), "statistics"),
    "group_boundary_channel": ("split", (2, 300, 320), "statistics"),
    "fused_idle_threads_live": ("fused", (1, 1632, 1280), "statistics"),
    "fused_last_pass_missing": ("fused", (1, 1632, 1280), "placement"),
    "apply_tail_rows_left": ("split", (2, 300, 320), "placement"),
    "gamma_beta_neighbour_octet": ("split", (2, 300, 320), "placement"),
    "tile_fold_stops_at_256": ("tile_sums", (1, 33280, 64, None), "statistics"),
    "tile_seam_pitch": ("tile_sums", (2, 512, 64, 24), "statistics"),
    "tile_producer_per_group": ("tile_sums", (2, 512, 256, 20), "statistics"),
    "ln_octets_beyond_64_missing": ("ln", (1034, 1032), "statistics"),
    "ln_rows_clamped_row_stored": ("ln_stats_rows", (8193 + 5, 320), "placement"),
    "ln_addvec_row_plus_one": ("ln_stats_rows", (8193 + 5, 320), "placement"),
}
