"""Operand patterns whose softmax is a 0/1 selection, for bit-exact tests of the attention kernels
(tests/test_attention_exact_gpu.py on the GPU, tests/test_exact_patterns_cpu.py for what they can see).

A pattern gives every query a set of SELECTED keys whose scores are bit-identical and every other key a score at least
GAP log2 units below.  Then every selected key has one common probability P0, every other key probability exactly zero, and
the output row is an integer mean the test knows: S / count with S the sum of the selected rows of V (non-zero integers in
[-7, 7], different per batch item, head, key and channel).

* ``uniform``  q = 0: every key selected.
* ``onehot``   key j carries a +-1 code of its index, query i carries G times the code of pi(i): row i is V[pi(i)].
* ``strided``  q_i = G e(i mod stride), k_j = e(j mod stride): query i selects the keys j = i (mod stride) -- one key of
               every K/V tile (stride = head_dim = 64), a different one per query.

GAP.  26 log2 units would make an fp16 probability exactly zero (2^-26 rounds to zero in fp16).  That covers a kernel whose P
is rounded to fp16 against the FINAL reference.  The kernels also hold fp32 quantities that must vanish: the online
softmax of csrc/attention.hip rescales what it summed before the selected key arrived by 2^-gap in fp32 (l and O of a first
tile without a selected key are of order 64 x 7), and ``attn_small_kernel`` (csrc/clip.hip) keeps P in fp32 throughout.  So G
is chosen for GAP = 160: 2^-160 is below fp32's smallest subnormal, and a product of order 2^-160 x 2^15 added to a sum
>= 1 leaves it as it was.  ``check_selection`` asserts the gap from the scores as the kernel forms them (for the spatial
kernels from the fp16-rounded, pre-scaled query, csrc/attention.hip:73).

Criterion (``violations``): x = S / count in fp64.
* where x is representable in fp16 the output equals it bit for bit (every one-hot row; uniform and strided rows with a
  power-of-two count and |S| <= 2,048);
* elsewhere the output is within one fp16 ulp of x: ``acc * (1 / l)`` rounds the reciprocal, the product and the fp16
  conversion;
* ``attn_temporal_kernel`` normalises P in fp32 and rounds P / l to fp16 BEFORE the P.V product (``v_cvt_f16_f32`` of
  ``pv * inv``, csrc/attention.hip:360): with a count that is no power of two, fp16(1 / count) is off by up to 2^-12
  relative and so is every output, representable quotient or not.  Those rows are held to one ulp (``p_rounded=True``).

Plain helper module: no fixtures, no tests."""
from __future__ import annotations

import math

import torch

LOG2E = 1.4426950408889634
GAP = 160.0
PATTERNS = ("uniform", "onehot", "strided")


def values(batch, hw, heads, keys, hd, seed=0):
    """V [batch][hw][heads][keys][hd]: seeded non-zero integers in [-7, 7] (fp32).  hw = 1 for the spatial kernels; the
    temporal kernel runs one sequence per (batch item, pixel, head)."""
    g = torch.Generator().manual_seed(1234 + seed)
    shape = (batch, hw, heads, keys, hd)
    return (torch.randint(1, 8, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def index_code(n, hd):
    """(+-1 code [n][hd] of the indices 0..n-1, dims per bit): bit b of j sits in dims [b r, (b + 1) r), unused dims are 0.
    Two different indices differ in at least r dims, so their dot product is at least 2 r below a code's own."""
    bits = max(1, (n - 1).bit_length())
    r = hd // bits
    assert r >= 1, f"{n} keys need {bits} bits, head_dim {hd} has no room"
    code = torch.zeros(n, hd)
    j = torch.arange(n)
    for b in range(bits):
        code[:, b * r:(b + 1) * r] = (((j >> b) & 1) * 2 - 1).float()[:, None]
    return code, r


def permutation(n, seed=0):
    """A seeded permutation of 0..n-1 with pi(0) = n - 1: it crosses every tile and block boundary and reaches the last key."""
    p = torch.randperm(n, generator=torch.Generator().manual_seed(77 + seed))
    i = int((p == n - 1).nonzero()[0])
    p[i], p[0] = p[0], n - 1
    return p


def power_of_two_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


def make(pattern, n, hd, scale, *, stride=None, pi=None, seed=0):
    """(q [n][hd], k [n][hd], sel [n queries][n keys] bool) for one sequence of n tokens; the same q and k serve every
    batch item and head (V differs).  G is a power of two, so q is exact in fp16."""
    if pattern == "uniform":
        g = torch.Generator().manual_seed(5 + seed)
        k = torch.randint(-3, 4, (n, hd), generator=g).float()           # any keys: q = 0 makes every score zero
        return torch.zeros(n, hd), k, torch.ones(n, n, dtype=torch.bool)
    if pattern == "onehot":
        code, r = index_code(n, hd)
        pi = permutation(n, seed) if pi is None else pi
        gain = power_of_two_at_least(GAP / (2 * r * scale * LOG2E) * 1.01)
        sel = torch.zeros(n, n, dtype=torch.bool)
        sel[torch.arange(n), pi] = True
        return gain * code[pi], code, sel
    if pattern == "strided":
        stride = hd if stride is None else stride
        assert stride <= hd
        eye = torch.eye(hd)[torch.arange(n) % stride]
        gain = power_of_two_at_least(GAP / (scale * LOG2E) * 1.01)
        sel = (torch.arange(n)[:, None] % stride) == (torch.arange(n)[None, :] % stride)
        return gain * eye, eye, sel
    raise ValueError(pattern)


def scores_log2(q, k, scale, kind):
    """The scores in log2 units as each kernel forms them (fp32)."""
    sl = torch.tensor(scale * LOG2E, dtype=torch.float32)
    q, k = q.half().float(), k.half().float()
    if kind == "spatial":                 # Q pre-multiplied by scale * log2 e, one rounding to fp16
        return (q * sl).half().float() @ k.t()
    if kind == "temporal":                # scaled after the product
        return (q @ k.t()) * sl
    if kind == "small":                   # q * scale in fp32, log2 e at the exponential
        return ((q * torch.tensor(scale, dtype=torch.float32)) @ k.t()) * torch.tensor(LOG2E, dtype=torch.float32)
    raise ValueError(kind)


def check_selection(q, k, sel, scale, kind):
    """Asserts what the criterion rests on: the selected scores of a row are bit-identical and the row's maximum, every
    other score is at least GAP below, and q, k are exact in fp16."""
    assert torch.equal(q.half().float(), q) and torch.equal(k.half().float(), k)
    s = scores_log2(q, k, scale, kind)
    top = s.amax(1, keepdim=True)
    assert torch.equal(torch.where(sel, s, top), top.expand_as(s)), "selected scores differ within a row"
    rest = torch.where(sel, torch.full_like(s, -float("inf")), s)
    assert float((top - rest).min()) >= GAP, f"an unselected key is only {float((top - rest).min()):.1f} log2 units below"
    assert bool(sel.any(1).all())


def expected(sel, v):
    """(S [...][n][hd] fp64, count [n]) and the model's 24-bit assertions (P0 = 1: numerator S, row sum count)."""
    count = sel.sum(1)
    s = torch.einsum("qk,...kd->...qd", sel.float(), v.float()).double()      # (integers below 2^24: exact in fp32)
    assert float(s.abs().max()) < 2 ** 24 and int(count.max()) < 2 ** 24
    return s, count


def fp16_ulp(x):
    """Spacing of fp16 at |x| (fp64 tensor; subnormal spacing below 2^-14)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def _held_bit_equal(x, count, p_rounded):
    rep = x.half().double() == x
    if p_rounded:
        rep = rep & ((count & (count - 1)) == 0)[:, None]
    return rep


def violations(got, s, count, p_rounded=False):
    """'' if ``got`` [batch][hw][heads][n][hd] meets the criterion, else a description of the first element that does not."""
    x = s / count.double()[:, None]
    got = got.double()
    rep = _held_bit_equal(x, count, p_rounded)
    bad = torch.where(rep, got != x, ~((got - x).abs() <= fp16_ulp(x)))
    bad = bad | ~torch.isfinite(got)
    if not bool(bad.any()):
        return ""
    at = tuple(int(t) for t in bad.nonzero()[0])
    rows = sorted(set(bad.nonzero()[:, -2].tolist()))
    return (f"{int(bad.sum())} values in query rows {rows[:5]}{'...' if len(rows) > 5 else ''} break the criterion; first at (batch, "
            f"pixel, head, query, channel) = {at}: got {float(got[at])!r}, S / count = {float(s[at])} / {int(count[at[-2]])} = "
            f"{float(x[at])!r} ({'must be bit-equal' if bool(rep[at]) else 'one ulp = %g' % float(fp16_ulp(x)[at])})")


def must_be_bit_equal(s, count, p_rounded=False):
    """Share of the outputs held bit-equal (the rest: one ulp)."""
    return float(_held_bit_equal(s / count.double()[:, None], count, p_rounded).double().mean())


# ------------------------------------------------------------------------------------------------ shapes
SPATIAL_SHORT = [6, 64, 65, 200, 576]              # 64-key tiles: one ragged tile, one whole, one + 1, ragged, several blocks
SPATIAL_MID = [1024, 1025, 1100, 1281]             # from 1,024 keys
SPATIAL_LONG = [4096, 4608]                        # sp_attn_spatial_long_f16's own shapes (multiples of 256 from 4,096)
TEMPORAL_FRAMES = [1, 14, 16, 17, 25, 32]
TEMPORAL_HW = [9, 37]
SMALL = [(1, 8), (65, 40), (257, 80), (280, 128), (512, 40)]


def temporal_stride(frames):
    """The smallest stride > 1 that divides ``frames`` (a prime count: the count itself, one key per query; 1 frame: 1)."""
    for s in range(2, frames + 1):
        if frames % s == 0:
            return s
    return 1


def near_map(n):
    """For the long kernel: pi(i) inside query i's own 256-block (mirrored), every seventh query into K/V tile 0."""
    i = torch.arange(n)
    own = (i // 256) * 256 + 255 - i % 256
    return torch.where(i % 7 == 0, i % 64, own)


def far_map(n, blocks):
    """near_map with the queries of ``blocks`` sent far: the first of them to the last 256 keys (mirrored: query 0 of the
    block reaches the last key), the others to keys 64.. of another block, outside their own block and outside tile 0."""
    pi = near_map(n)
    for j, blk in enumerate(blocks):
        i = torch.arange(blk * 256, blk * 256 + 256)
        if j == 0:
            assert blk != n // 256 - 1
            pi[i] = n - 1 - (i - blk * 256)
        else:
            assert blk >= 2
            pi[i] = 64 + (i - blk * 256)
    return pi


# ------------------------------------------------------------------------------------------------ buffers
# Rows are ordered (batch item, token, pixel): row = (b n + t) hw + p.  hw = 1 is the spatial layout, hw > 1 the temporal
# one (token = frame).  q and k are the same for every batch item, pixel and head; V differs in all of them.
SLACK = 8


def rows_of(q, k, v):
    """q, k [n][hd], v [batch][hw][heads][n][hd] -> three [rows][heads hd] fp32 matrices."""
    batch, hw, heads, n, hd = v.shape
    c = heads * hd
    qq = q[None, :, None, None, :].expand(batch, n, hw, heads, hd).reshape(batch * n * hw, c)
    kk = k[None, :, None, None, :].expand(batch, n, hw, heads, hd).reshape(batch * n * hw, c)
    return qq, kk, v.permute(0, 3, 1, 2, 4).reshape(batch * n * hw, c)


def sequences(rows, batch, hw, heads, n, hd):
    """[rows][heads hd] -> [batch][hw][heads][n][hd]."""
    return rows.reshape(batch, n, hw, heads, hd).permute(0, 2, 3, 1, 4)


def pack(qq, kk, vv):
    """One wide fp16 buffer with q, k, v as column slices and SLACK NaN columns in front of, between and behind them:
    (buffer [rows][3 (c + SLACK) + SLACK], [q columns, k columns, v columns])."""
    c = qq.shape[1]
    buf = torch.full((qq.shape[0], 3 * (c + SLACK) + SLACK), float("nan"), dtype=torch.float16)
    cols = [slice(SLACK + j * (c + SLACK), SLACK + j * (c + SLACK) + c) for j in range(3)]
    for sl, t in zip(cols, (qq, kk, vv)):
        buf[:, sl] = t.half()
    return buf, cols


# ------------------------------------------------------------------------------------------------ CPU models and mutants
# fp32 statements of the three kernels' rounding points (tests/test_kernels_gpu.py: _spatial_statement, _temporal_statement;
# csrc/clip.hip), run on the SAME flat rows the GPU tests pass, with plausible indexing bugs planted on request.
MUTANTS = ("last key ignored", "key 64 read from key 63", "key 256 read from key 255", "zero row behind the last key counted",
           "head 1 reads head 0's V", "batch item 1 starts one row early", "two V channels of one lane swapped",
           "last query row of a block copies the row before")


def applies(mutant, kind, batch, hw, heads, n):
    """Where a mutant has something to act on.  A row behind the last key exists only in a ragged last tile (64 keys; 16
    frames in the temporal kernel): with whole tiles the kernels mask nothing."""
    return {"last key ignored": n >= 2, "key 64 read from key 63": n > 64, "key 256 read from key 255": n > 256,
            "zero row behind the last key counted": n % (16 if kind == "temporal" else 64) != 0,
            "head 1 reads head 0's V": heads >= 2, "batch item 1 starts one row early": batch >= 2,
            "last query row of a block copies the row before": n >= 2}.get(mutant, True)


def _tiled(q, k, v, sl):
    """csrc/attention.hip / attention_long.hip: [X][n][hd] problems, 64-key tiles, running reference raised past +8."""
    s = (q * sl).half().float() @ k.transpose(-1, -2)
    m = l = o = None
    for t0 in range(0, s.shape[-1], 64):
        st = s[..., t0:t0 + 64]
        mt = st.amax(-1, keepdim=True)
        if t0 == 0:
            m, l, o = mt, torch.zeros_like(mt), torch.zeros(q.shape[:-1] + v.shape[-1:])
        else:
            delta = torch.where(mt - m > 8.0, mt - m, torch.zeros_like(mt))
            m, l, o = m + delta, l * torch.exp2(-delta), o * torch.exp2(-delta)
        p16 = torch.exp2(st - m).half().float()
        l = l + p16.sum(-1, keepdim=True)
        o = o + p16 @ v[..., t0:t0 + 64, :]
    return (o * (1.0 / l)).half()


def _temporal(q, k, v, sl):
    s = q @ k.transpose(-1, -2)
    p = torch.exp2(s * sl - s.amax(-1, keepdim=True) * sl)
    p16 = (p * (1.0 / p.sum(-1, keepdim=True))).half().float()
    return (p16 @ v).half()


def _small(q, k, v, scale):
    s = (q * torch.tensor(scale, dtype=torch.float32)) @ k.transpose(-1, -2)
    p = torch.exp2((s - s.amax(-1, keepdim=True)) * torch.tensor(LOG2E, dtype=torch.float32))
    return ((p @ v) * (1.0 / p.sum(-1, keepdim=True))).half()


def model(kind, qq, kk, vv, batch, hw, heads, n, hd, scale, mutant=None):
    """The kernel ``kind`` ('spatial', 'temporal', 'small') on flat rows -> [batch][hw][heads][n][hd] fp32."""
    qq, kk, vv = [t.half().float() for t in (qq, kk, vv)]
    if mutant == "batch item 1 starts one row early":
        per = n * hw
        qq, kk, vv = [torch.cat([t[:per], t[per - 1:2 * per - 1], t[2 * per:]]) for t in (qq, kk, vv)]
    q, k, v = [sequences(t, batch, hw, heads, n, hd).reshape(-1, n, hd).clone() for t in (qq, kk, vv)]
    if mutant == "head 1 reads head 0's V":
        v5 = v.reshape(batch, hw, heads, n, hd)
        v5[:, :, 1] = v5[:, :, 0]
    if mutant == "last key ignored":
        k, v = k[:, :-1], v[:, :-1]
    for edge in (64, 256):
        if mutant == f"key {edge} read from key {edge - 1}":
            k[:, edge], v[:, edge] = k[:, edge - 1], v[:, edge - 1]
    if mutant == "zero row behind the last key counted":
        k, v = [torch.cat([t, torch.zeros(t.shape[0], 1, hd)], dim=1) for t in (k, v)]
    sl = torch.tensor(scale * LOG2E, dtype=torch.float32)
    step = max(1, int(6e7 // (n * k.shape[1])))
    out = torch.cat([{"spatial": _tiled, "temporal": _temporal}[kind](q[i:i + step], k[i:i + step], v[i:i + step], sl) if kind != "small"
                     else _small(q[i:i + step], k[i:i + step], v[i:i + step], scale) for i in range(0, q.shape[0], step)]).float()
    if mutant == "two V channels of one lane swapped":
        lane = torch.arange(n) % 32 == min(7, n - 1)
        out[:, lane] = out[:, lane][..., [0, 1, 3, 2] + list(range(4, hd))]
    if mutant == "last query row of a block copies the row before":
        for i in {n - 1, min(n, 128) - 1}:
            out[:, i] = out[:, i - 1]
    return out.reshape(batch, hw, heads, n, hd)
