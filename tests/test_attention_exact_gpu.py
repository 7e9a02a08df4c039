"""Bit-exact parity of the attention kernels on operands whose softmax is a 0/1 selection (tests/attention_patterns.py:
``uniform``, ``onehot``, ``strided``; the criterion -- bit-equal where the integer mean is representable in fp16, one fp16 ulp
elsewhere -- and its reasons are in that module's docstring).  A lost, doubled or misplaced key, a wrong head or batch stride
or a swapped channel is a wrong integer, at any sequence length (tests/test_exact_patterns_cpu.py plants them).

Every call takes q, k and v as column slices of one wide buffer whose other columns are NaN and writes an output slice
between guard rows and guard columns; V differs per batch item, pixel, head, key and channel.

sp_attn_spatial_long_f16 runs at both sp_attn_long_set_occupancy settings.  Patterns whose selected keys lie in every tile,
in the query's own 256-block or in K/V tile 0 must leave every flag word zero (the frozen-reference kernel produced the
bytes); the one-hot pattern with far keys must flag exactly the blocks whose queries look far, and still be exact.

Held to one ulp instead of bit-equality: sp_attn_temporal_f16 where the number of selected keys is no power of two (it
rounds P / l to fp16 before the P.V product: ``v_cvt_f16_f32`` of ``pv * inv``, csrc/attention.hip:360)."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_patterns as P  # noqa: E402

DEV = "cuda"
GUARD = 2
NAMES = {1: "attn_long_kernel<2, 1>", 2: "attn_long_kernel<2, 2>"}


@pytest.fixture
def ops():
    from vdpp_amd.hip import ops
    yield ops
    ops.attn_long_set_occupancy(0)


def run(call, q, k, v):
    """Packs (q, k [n][hd]; v [batch][hw][heads][n][hd]), calls ``call(qs, ks, vs, out, ld, ldo)`` on the device slices and
    returns the output as [batch][hw][heads][n][hd] after checking the guards."""
    batch, hw, heads, n, hd = v.shape
    c = heads * hd
    buf, cols = P.pack(*P.rows_of(q, k, v))
    dev = buf.to(DEV)
    rows = buf.shape[0]
    obuf = torch.full((rows + 2 * GUARD, c + 2 * P.SLACK), float("nan"), dtype=torch.float16, device=DEV)
    out = obuf[GUARD:GUARD + rows, P.SLACK:P.SLACK + c]
    call(dev[:, cols[0]], dev[:, cols[1]], dev[:, cols[2]], out, buf.shape[1], obuf.stride(0))
    torch.cuda.synchronize()
    got = obuf.cpu()
    assert torch.isnan(got[:GUARD]).all() and torch.isnan(got[GUARD + rows:]).all(), "guard rows written"
    assert torch.isnan(got[:, :P.SLACK]).all() and torch.isnan(got[:, P.SLACK + c:]).all(), "guard columns written"
    return P.sequences(got[GUARD:GUARD + rows, P.SLACK:P.SLACK + c].float(), batch, hw, heads, n, hd)


def judge(got, sel, v, what, p_rounded=False):
    s, count = P.expected(sel, v)
    bad = P.violations(got, s, count, p_rounded)
    assert not bad, f"{what}: {bad}"
    return P.must_be_bit_equal(s, count, p_rounded)


def spatial_case(pattern, seq, **kw):
    q, k, sel = P.make(pattern, seq, 64, 0.125, **kw)
    P.check_selection(q, k, sel, 0.125, "spatial")
    return q, k, sel


@pytest.mark.parametrize("pattern", P.PATTERNS)
@pytest.mark.parametrize("seq", P.SPATIAL_SHORT + P.SPATIAL_MID)
def test_attention_spatial_exact(ops, seq, pattern):
    batch, heads = (1 if seq == 1025 else 2), 2
    q, k, sel = spatial_case(pattern, seq)
    v = P.values(batch, 1, heads, seq, 64, seed=seq)
    got = run(lambda qs, ks, vs, o, ld, ldo: ops.attn_spatial(qs, ks, vs, o, ldq=ld, ldk=ld, ldv=ld, ldo=ldo, batch=batch, seq=seq,
                                                              heads=heads), q, k, v)
    share = judge(got, sel, v, f"sp_attn_spatial_f16 {pattern} seq {seq}")
    print(f"spatial {pattern} seq {seq}: {share:.0%} of the outputs held bit-equal")
    if pattern == "onehot" or (seq & (seq - 1)) == 0 and pattern == "uniform":
        assert share == 1.0


@functools.lru_cache(maxsize=None)
def long_case(pattern, seq):
    """Operands and the expected sums, computed once for both occupancy settings (and left unchanged)."""
    nblk = seq // 256
    far = (1, nblk - 2) if pattern == "onehot_far" else ()
    if pattern.startswith("onehot"):
        q, k, sel = spatial_case("onehot", seq, pi=P.far_map(seq, far))
    else:
        q, k, sel = spatial_case(pattern, seq)
    v = P.values(2, 1, 2, seq, 64, seed=seq)
    return q, k, v, P.expected(sel, v), list(far)


def _long(ops, occ, q, k, v, seq):
    batch, heads = v.shape[0], v.shape[2]
    ws = torch.full((ops.attn_long_ws_bytes(batch, seq, heads) // 4,), 0x7fffffff, dtype=torch.int32, device=DEV)   # stale junk
    ops.attn_long_set_occupancy(occ)
    got = run(lambda qs, ks, vs, o, ld, ldo: ops.attn_spatial_long(qs, ks, vs, o, ws, ldq=ld, ldk=ld, ldv=ld, ldo=ldo, batch=batch,
                                                                   seq=seq, heads=heads), q, k, v)
    assert ops.attn_long_last_kernel() == NAMES[occ]
    nblk = seq // 256
    words = ws.cpu()
    return got, words[:batch * heads * nblk].view(batch, heads, nblk), int(words[batch * heads * nblk])


@pytest.mark.parametrize("occ", [1, 2])
@pytest.mark.parametrize("pattern", ["uniform", "strided", "onehot_near", "onehot_far"])
@pytest.mark.parametrize("seq", P.SPATIAL_LONG)
def test_attention_spatial_long_exact(ops, seq, pattern, occ):
    q, k, v, (s, count), far = long_case(pattern, seq)
    got, flags, waves = _long(ops, occ, q, k, v, seq)
    bad = P.violations(got, s, count)
    assert not bad, f"sp_attn_spatial_long_f16 {pattern} seq {seq} occupancy {occ}: {bad}"
    share = P.must_be_bit_equal(s, count)
    # q and k are the same for every (batch item, head): the far blocks overflow the frozen reference in all four
    expect = torch.zeros_like(flags)
    expect[:, :, far] = 1
    assert torch.equal(flags, expect), f"flagged blocks {flags.nonzero().tolist()} expected {expect.nonzero().tolist()}"
    assert (waves > 0) == bool(far) and waves <= 4 * int(expect.sum())
    print(f"long {pattern} seq {seq} occupancy {occ}: {share:.0%} of the outputs held bit-equal, {int(flags.sum())} blocks flagged")


@pytest.mark.parametrize("pattern", P.PATTERNS)
@pytest.mark.parametrize("hw", P.TEMPORAL_HW)
@pytest.mark.parametrize("frames", P.TEMPORAL_FRAMES)
def test_attention_temporal_exact(ops, frames, hw, pattern):
    batch, heads = 2, 2
    q, k, sel = P.make(pattern, frames, 64, 0.125, stride=P.temporal_stride(frames))
    P.check_selection(q, k, sel, 0.125, "temporal")
    v = P.values(batch, hw, heads, frames, 64, seed=frames * 100 + hw)
    got = run(lambda qs, ks, vs, o, ld, ldo: ops.attn_temporal(qs, ks, vs, o, ldq=ld, ldk=ld, ldv=ld, ldo=ldo, batch=batch,
                                                               frames=frames, hw=hw, heads=heads), q, k, v)
    share = judge(got, sel, v, f"sp_attn_temporal_f16 {pattern} frames {frames} hw {hw}", p_rounded=True)
    print(f"temporal {pattern} frames {frames} hw {hw}: {share:.0%} of the outputs held bit-equal")
    if pattern == "onehot":
        assert share == 1.0


@pytest.mark.parametrize("pattern", P.PATTERNS)
@pytest.mark.parametrize("seq,hd", P.SMALL)
def test_attention_small_exact(ops, seq, hd, pattern):
    batch, heads = 2, 2
    scale = hd ** -0.5
    q, k, sel = P.make(pattern, seq, hd, scale, stride=min(hd, 64))
    P.check_selection(q, k, sel, scale, "small")
    v = P.values(batch, 1, heads, seq, hd, seed=seq + hd)
    got = run(lambda qs, ks, vs, o, ld, ldo: ops.attn_small(qs, ks, vs, o, ldq=ld, ldk=ld, ldv=ld, ldo=ldo, batch=batch, seq=seq,
                                                            heads=heads, head_dim=hd, scale=scale), q, k, v)
    share = judge(got, sel, v, f"sp_attn_small_f16 {pattern} seq {seq} head_dim {hd}")
    print(f"small {pattern} seq {seq} head_dim {hd}: {share:.0%} of the outputs held bit-equal")
    if pattern == "onehot":
        assert share == 1.0
