"""csrc/attention_temporal_long.hip: ``sp_attn_temporal_long_f16`` (33 .. 128 frames) against an fp64 softmax on the same
fp16 operands within the bound of ``sp_attn_temporal_f16``, whose arithmetic contract it keeps; per row on peaked logits with
dominant keys on both sides of every 16- and 32-frame seam; bit for bit on 0/1 selections; the refusals."""
import pytest
import torch

from tests import attention_patterns as P
from tests.test_kernels_gpu import _attn_fp64, _ops, _per_row_err, check, h, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _statement(q, k, v, scale=0.125):
    """The kernel's rounding points: fp32 scores scaled AFTER the product, P / l rounded to fp16, fp32 sums, fp16 output."""
    sl = torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    s = q @ k.transpose(-1, -2)
    p = torch.exp2(s * sl - s.amax(-1, keepdim=True) * sl)
    return ((p * (1.0 / p.sum(-1, keepdim=True))).half().float() @ v).half()


def _run(q, k, v):
    """q, k, v [batch][hw][heads][frames][64] (fp16-exact fp32) -> the kernel's output in the same layout.  q/k/v are column
    slices of one fused [rows + 1][3c] buffer whose last row is a NaN guard; the output is a slice of a wider NaN buffer."""
    batch, hw, heads, frames, _ = q.shape
    c, rows = heads * 64, batch * frames * hw
    qkv = torch.full((rows + 1, 3 * c), float("nan"), dtype=torch.float16)
    qkv[:rows] = torch.cat([t.permute(0, 3, 1, 2, 4).reshape(rows, c) for t in (q, k, v)], dim=1).half()
    d = qkv.to(DEV)
    obuf = torch.full((rows + 2, c + 16), float("nan"), dtype=torch.float16, device=DEV)
    _ops().attn_temporal_long(d[:rows, :c], d[:rows, c:2 * c], d[:rows, 2 * c:], obuf[1:-1, 8:8 + c], ldq=3 * c, ldk=3 * c,
                              ldv=3 * c, ldo=c + 16, batch=batch, frames=frames, hw=hw, heads=heads)
    got = obuf.cpu()
    assert torch.isnan(got[0]).all() and torch.isnan(got[-1]).all(), "rows outside o written"
    assert torch.isnan(got[:, :8]).all() and torch.isnan(got[:, 8 + c:]).all(), "pitch slack written"
    return got[1:-1, 8:8 + c].float().reshape(batch, frames, hw, heads, 64).permute(0, 2, 3, 1, 4)


@pytest.mark.parametrize("batch,hw,heads", [(1, 37, 3), (2, 5, 2)])
@pytest.mark.parametrize("frames", [33, 48, 64, 65, 96, 97, 128])
def test_attn_temporal_long_matches_fp64_softmax(frames, batch, hw, heads):
    """Both ends of every instantiation (64 / 96 / 128 keys), ragged last query block and key tile; 111 and 20 problems (a
    dead wave in the last workgroup); the second video starts at a row that is no multiple of 16."""
    g = torch.Generator().manual_seed(frames * hw)
    q, k, v = [h(torch.randn(batch, hw, heads, frames, 64, generator=g)) for _ in range(3)]
    got, ref = _run(q, k, v), _attn_fp64(q, k, v).float()
    print(f"attn_temporal_long {batch} x {frames} x {hw}, {heads} heads: rel-L2 {rel_l2(got, ref):.2e}")
    check(got, ref, l2=3e-3, mx=2e-2)


@pytest.mark.parametrize("amp", [1, 3, 6])
@pytest.mark.parametrize("frames", [33, 64, 97, 128])
def test_attn_temporal_long_peaked_rows_judged_per_row(frames, amp):
    """Logits of standard deviation amp^2; dominant keys (k = 1.5 x another frame's q) at frame 0, the last frame and both sides
    of every 16- and 32-frame seam that exists; one all-equal row (q = 0).  Bound per row: 3 x the statement's worst row."""
    g = torch.Generator().manual_seed(frames * 10 + amp)
    q, k, v = [h(torch.randn(1, 37, 3, frames, 64, generator=g) * a) for a in (amp, amp, 1)]
    planted = sorted({0, frames - 1, 15, 16, 31, 32, 63, 64, 95, 96} & set(range(frames)))
    for j, kf in enumerate(planted):                                  # pixel j, head 0: query frame kf + 3 finds key frame kf
        k[0, j, 0, kf] = h(1.5 * q[0, j, 0, (kf + 3) % frames])
    q[0, 5, 1, frames // 2] = 0.0
    ref = _attn_fp64(q, k, v)
    p = torch.softmax(q.double() @ k.double().transpose(-1, -2) * 0.125, dim=-1)
    assert all(float(p[0, j, 0, (kf + 3) % frames, kf]) > 0.9 for j, kf in enumerate(planted)), "a planted key does not dominate"
    bound = 3.0 * float(_per_row_err(_statement(q, k, v), ref).max())
    got = _run(q, k, v)
    err = _per_row_err(got, ref)
    print(f"attn_temporal_long peaked, {frames} frames, amplitude {amp}: worst row {float(err.max()):.2e}, bound {bound:.2e}")
    assert torch.isfinite(got).all() and float(err.max()) <= bound, f"worst row {float(err.max()):.3e} (row {int(err.argmax())}) > {bound:.3e}"


@pytest.mark.parametrize("pattern", ["onehot", "uniform", "strided"])
@pytest.mark.parametrize("frames", [64, 128])
def test_attn_temporal_long_exact_selections(frames, pattern):
    """tests/attention_patterns.py at 64 and 128 frames: one key per query, all keys, every second key -- counts 1, frames and
    frames / 2, all powers of two, so P / l is exact in fp16 and every representable integer mean is held bit for bit."""
    batch, hw, heads = 2, 9, 2
    q, k, sel = P.make(pattern, frames, 64, 0.125, stride=P.temporal_stride(frames))
    P.check_selection(q, k, sel, 0.125, "temporal")
    v = P.values(batch, hw, heads, frames, 64, seed=frames * 100 + hw)
    s, count = P.expected(sel, v)
    bad = P.violations(_run(q.expand(batch, hw, heads, frames, 64), k.expand(batch, hw, heads, frames, 64), v), s, count, p_rounded=True)
    assert not bad, f"sp_attn_temporal_long_f16 {pattern} frames {frames}: {bad}"
    assert pattern != "onehot" or P.must_be_bit_equal(s, count, p_rounded=True) == 1.0


@pytest.mark.parametrize("bad", [dict(frames=32), dict(frames=129), dict(ldk=64), dict(off=4)], ids=str)
def test_attn_temporal_long_refusals(bad):
    """Refused with the entry point's name, nothing written: frames, a pitch below heads*64 = 128, k 8 bytes off alignment."""
    frames, c = bad.get("frames", 40), 128
    d = torch.zeros(260, 3 * c, dtype=torch.float16, device=DEV)
    o = torch.full((260, c), 5.0, dtype=torch.float16, device=DEV)
    with pytest.raises(_ops().HipKernelError, match="sp_attn_temporal_long_f16"):
        _ops().attn_temporal_long(d[:, :c], d[:, c + bad.get("off", 0):], d[:, 2 * c:], o, ldq=3 * c, ldk=bad.get("ldk", 3 * c),
                                  ldv=3 * c, ldo=c, batch=1, frames=frames, hw=2, heads=2)
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())
