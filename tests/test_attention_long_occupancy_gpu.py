"""The two instantiations of the frozen-reference attention kernel (csrc/attention_long.hip): attn_long_kernel<2, 1>, one
workgroup per CU, and attn_long_kernel<2, 2>, which fits 256 registers per wave so that two workgroups share a CU.  The
second runs the warm-up's two query blocks one after the other instead of interleaved; a block's arithmetic does not
depend on the other block, so the outputs must be the same BYTES, not merely close.

Shape: seq = 4096 is the smallest the host contract admits (64 K/V tiles, 16 workgroups per (item, head): the first and
the last own-tile positions both occur).  Tolerances are those of tests/test_kernels_gpu.py: 3e-3 / 2e-2 against fp32
attention (test_attention_spatial_long), 2e-3 / 1e-2 against the ordinary kernel (test_attention_spatial_long_second_pass)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
L2_FP32, MX_FP32 = 3e-3, 2e-2          # test_attention_spatial_long
L2_ORD, MX_ORD = 2e-3, 1e-2            # test_attention_spatial_long_second_pass, against the ordinary kernel
NAMES = {1: "attn_long_kernel<2, 1>", 2: "attn_long_kernel<2, 2>"}


@pytest.fixture
def ops():
    from vdpp_amd.hip import ops
    yield ops
    ops.attn_long_set_occupancy(0)


def h(t):  # fp16-rounded fp32 copy (what the kernel actually sees)
    return t.half().float()


def check(out, ref, l2, mx):
    out = out.float().cpu()
    assert torch.isfinite(out).all()
    e = float((out.double() - ref.double()).norm() / ref.double().norm())
    m = float((out - ref).abs().max() / ref.abs().max())
    assert e <= l2 and m <= mx, f"rel_l2={e:.3e} max_rel={m:.3e}"


def run(ops, occ, d, c, batch, seq, heads):
    """q/k/v are column slices of one [rows][3c] buffer (ld = 3c), as the engine passes them"""
    o = torch.empty(batch * seq, c, dtype=torch.float16, device=DEV)
    ws = torch.full((ops.attn_long_ws_bytes(batch, seq, heads) // 4,), 0x7fffffff, dtype=torch.int32, device=DEV)
    ops.attn_long_set_occupancy(occ)
    ops.attn_spatial_long(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o, ws, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c,
                          batch=batch, seq=seq, heads=heads)
    assert ops.attn_long_last_kernel() == NAMES[occ]
    return o, ws


def sdpa(qkv, c, batch, seq, heads):
    q, k, v = [t.reshape(batch, seq, heads, 64).transpose(1, 2) for t in qkv.split(c, dim=1)]
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(batch * seq, c)


@pytest.mark.parametrize("batch,seq,heads", [(1, 4096, 1), (2, 4096, 2)])
def test_two_workgroups_per_cu_is_bit_identical(ops, batch, seq, heads):
    c = heads * 64
    g = torch.Generator().manual_seed(seq + batch + heads)
    d = torch.randn(batch * seq, 3 * c, generator=g).half().to(DEV)
    o1, ws1 = run(ops, 1, d, c, batch, seq, heads)
    o2, ws2 = run(ops, 2, d, c, batch, seq, heads)
    assert torch.equal(o1, o2)
    assert torch.equal(ws1, ws2)
    assert int(ws2.sum()) == 0          # unit-variance rows stay within 16 of their warm-up maximum: what was compared is
                                        # the frozen-reference kernel's own output, not the second pass's


def test_two_workgroups_per_cu_against_fp32(ops):
    batch, seq, heads = 1, 4096, 1
    c = heads * 64
    g = torch.Generator().manual_seed(seq + heads)
    qkv = h(torch.randn(batch * seq, 3 * c, generator=g))
    o, ws = run(ops, 2, qkv.half().to(DEV), c, batch, seq, heads)
    assert int(ws.sum()) == 0
    check(o, sdpa(qkv, c, batch, seq, heads), L2_FP32, MX_FP32)


def test_two_workgroups_per_cu_second_pass_repairs(ops):
    """A few keys far from their queries score > 16 log2-units above the warm-up maximum (2.5 x the query: ~ +29 against
    ~5): their 256-row blocks overflow the frozen reference and are recomputed, the others are not."""
    batch, seq, heads = 2, 4096, 2
    c = heads * 64
    nblk = seq // 256
    g = torch.Generator().manual_seed(11)
    qkv = h(torch.randn(batch * seq, 3 * c, generator=g))
    q, k = qkv[:, :c].view(batch, seq, heads, 64), qkv[:, c:2 * c].view(batch, seq, heads, 64)
    expect = torch.zeros(batch, heads, nblk, dtype=torch.int32)
    for b, hd, qrow, krow in [(1, 0, 700, 3000), (0, 1, 3900, 1200), (0, 0, 40, 2500)]:
        k[b, krow, hd] = h(q[b, qrow, hd] * 2.5)
        expect[b, hd, qrow // 256] = 1
    qkv = h(qkv)
    d = qkv.half().to(DEV)
    o, ws = run(ops, 2, d, c, batch, seq, heads)
    flags = ws.cpu()[:batch * heads * nblk].view(batch, heads, nblk)
    flagged = int(flags.sum())
    assert 0 < flagged < batch * heads * nblk
    assert torch.equal(flags, expect), f"flagged blocks {flags.nonzero().tolist()} expected {expect.nonzero().tolist()}"
    waves = int(ws.cpu()[batch * heads * nblk])
    assert 0 < waves <= 4 * flagged
    o_ord = torch.empty_like(o)
    ops.attn_spatial(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o_ord, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, batch=batch,
                     seq=seq, heads=heads)
    check(o, o_ord.float().cpu(), L2_ORD, MX_ORD)
    check(o, sdpa(qkv, c, batch, seq, heads), L2_FP32, MX_FP32)
    # the other arm: same bytes, same blocks (the flagged-waves word may differ: <2, 2> gives a block up at the first look
    # after one of its waves overflowed, before the others might)
    o1, ws1 = run(ops, 1, d, c, batch, seq, heads)
    assert torch.equal(o1, o) and torch.equal(ws1[:batch * heads * nblk], ws[:batch * heads * nblk])


def test_occupancy_hook_names_what_ran(ops):
    c = 64
    d = torch.randn(4096, 3 * c, generator=torch.Generator().manual_seed(3)).half().to(DEV)
    for occ in (1, 2):
        run(ops, occ, d, c, 1, 4096, 1)
    ops.attn_long_set_occupancy(0)
    o = torch.empty(4096, c, dtype=torch.float16, device=DEV)
    ws = torch.zeros(ops.attn_long_ws_bytes(1, 4096, 1) // 4, dtype=torch.int32, device=DEV)
    kw = dict(ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, batch=1, heads=1)
    ops.attn_spatial_long(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o, ws, seq=4096, **kw)
    assert ops.attn_long_last_kernel() == NAMES[2]           # the library's default
    ops.attn_spatial_long(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o, ws, seq=2304, **kw)      # not this kernel's shape
    assert ops.attn_long_last_kernel() == "attn_spatial_kernel"
    with pytest.raises(ops.HipKernelError, match="occ"):
        ops.attn_long_set_occupancy(3)
