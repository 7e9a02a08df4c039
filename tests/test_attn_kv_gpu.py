"""csrc/attention_kv.hip: ``sp_kv_pool_f16`` bit for bit against torch's fp32 cell mean, ``sp_attn_spatial_kv_f16`` against an
fp64 softmax on the same fp16 operands (the bound ``sp_attn_spatial_f16`` is held to), per row on peaked logits whose row
maximum rises in every key tile, and the refusals."""
import pytest
import torch

from tests.attention_patterns import kv_statement as _kv_statement      # (the kernel's rounding points; shared with the CPU mutants)
from tests.test_kernels_gpu import _attn_fp64, _per_row_err, check, h, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vdpp_amd.hip import ops
    return ops


@pytest.mark.parametrize("n_img,gh,gw,f,c", [(2, 4, 6, 2, 64), (1, 8, 8, 4, 128), (3, 2, 2, 2, 320)])
def test_kv_pool_is_the_fp32_cell_mean_bit_for_bit(n_img, gh, gw, f, c):
    """Inputs are multiples of 2^-6 with |x| <= 4: every partial sum is exact in fp32, so the order of summation is free."""
    g = torch.Generator().manual_seed(gh * gw + c)
    qkv = (torch.randint(-256, 257, (n_img * gh * gw, 3 * c), generator=g).float() / 64).half()
    want = [qkv[:, i * c:(i + 1) * c].float().view(n_img, gh // f, f, gw // f, f, c).mean((2, 4)).reshape(-1, c).half() for i in (1, 2)]
    d = qkv.to(DEV)
    rows, pitch = n_img * (gh // f) * (gw // f), c + 24
    out = [torch.full((rows, pitch), float("nan"), dtype=torch.float16, device=DEV) for _ in range(2)]
    _ops().kv_pool(d[:, c:2 * c], d[:, 2 * c:], out[0], out[1], ldk=3 * c, ldv=3 * c, ldkp=pitch, ldvp=pitch, n_img=n_img, h=gh,
                   w=gw, c=c, factor=f)
    for got, ref in zip(out, want):
        assert torch.equal(got[:, :c].cpu().view(torch.int16), ref.view(torch.int16))
        assert torch.isnan(got[:, c:]).all(), "pitch slack written"


def _run(q, k, v):
    """q [batch][heads][seq_q][64], k, v [batch][heads][seq_kv][64] (fp16-exact fp32) -> the kernel's o in the same layout.
    Three buffers, three pitches, NaN guard rows around o."""
    batch, heads, seq_q, _ = q.shape
    seq_kv, c = k.shape[2], heads * 64
    bufs = []
    for t, pad in ((q, 8), (k, 64), (v, 136)):
        rows = t.permute(0, 2, 1, 3).reshape(-1, c)
        buf = torch.full((rows.shape[0], c + pad), 7.0, dtype=torch.float16, device=DEV)
        buf[:, :c] = rows.half().to(DEV)
        bufs.append(buf)
    o = torch.full((batch * seq_q + 16, c), float("nan"), dtype=torch.float16, device=DEV)
    _ops().attn_spatial_kv(bufs[0], bufs[1], bufs[2], o[8:-8], ldq=c + 8, ldk=c + 64, ldv=c + 136, ldo=c, batch=batch,
                           seq_q=seq_q, seq_kv=seq_kv, heads=heads)
    assert torch.isnan(o[:8]).all() and torch.isnan(o[-8:]).all(), "rows outside o written"
    return o[8:-8].float().cpu().view(batch, seq_q, heads, 64).permute(0, 2, 1, 3)


@pytest.mark.parametrize("batch,seq_q,seq_kv,heads", [(1, 72, 18, 1), (2, 320, 80, 2), (1, 576, 144, 5), (3, 256, 576, 1),
                                                      (1, 130, 1, 1)])
def test_attn_spatial_kv_matches_fp64_softmax(batch, seq_q, seq_kv, heads):
    g = torch.Generator().manual_seed(seq_q + seq_kv)
    q = h(torch.randn(batch, heads, seq_q, 64, generator=g))
    k, v = [h(torch.randn(batch, heads, seq_kv, 64, generator=g)) for _ in range(2)]
    got, ref = _run(q, k, v), _attn_fp64(q, k, v).float()
    print(f"attn_spatial_kv {batch} x {seq_q} x {seq_kv}, {heads} heads: rel-L2 {rel_l2(got, ref):.2e}")
    check(got, ref, l2=3e-3, mx=2e-2)
    if seq_kv == 1:
        assert torch.equal(got, v.expand_as(got)), "one key: every output row is that V row"


def test_attn_spatial_kv_peaked_rows_judged_per_row():
    """(1, 576, 144, 5) with logits of standard deviation about 4 and, along one channel, a key component that grows with
    the key index (0.25 per key in the logit: 16 per tile), so the row maximum rises in the second tile for every row and
    in the 16-key tail for nine rows in ten, and O and l are rescaled there.  Worst row within 3 x the worst row of the
    statement above, as for sp_attn_spatial_f16."""
    g = torch.Generator().manual_seed(9)
    q = torch.randn(1, 5, 576, 64, generator=g) * 4
    k, v = torch.randn(1, 5, 144, 64, generator=g), torch.randn(1, 5, 144, 64, generator=g)
    q[..., 0] = 4.0
    k[..., 0] = 0.5 * torch.arange(144.0)
    q, k, v = h(q), h(k), h(v)
    ref = _attn_fp64(q, k, v)
    logits = (q @ k.transpose(-1, -2) * 0.125)
    tile_max = [logits[..., t0:t0 + 64].amax(-1) for t0 in (0, 64, 128)]
    assert (tile_max[1] > tile_max[0]).float().mean() > 0.99 and (tile_max[2] > tile_max[1]).float().mean() > 0.85
    own = float(_per_row_err(_kv_statement(q, k, v), ref).max())
    err = _per_row_err(_run(q, k, v), ref)
    print(f"attn_spatial_kv peaked rows: logit std {float(logits.std()):.1f}, worst row {float(err.max()):.2e}, the statement's own {own:.2e}")
    assert float(err.max()) <= 3.0 * own, f"worst row {float(err.max()):.3e} (row {int(err.argmax())}) > 3 x {own:.3e}"


POOL_OK = dict(k=0, v=0, ldk=192, ldv=192, kp=0, vp=0, ldkp=64, ldvp=64, n_img=1, h=4, w=4, c=64, factor=2)
ATTN_OK = dict(q=0, k=0, v=0, o=0, ldq=64, ldk=64, ldv=64, ldo=64, batch=1, seq_q=16, seq_kv=4, heads=1, scale=0.125)
REFUSED = [("pool", dict(k=None)), ("pool", dict(vp=None)), ("pool", dict(factor=3)), ("pool", dict(factor=1)), ("pool", dict(h=5)),
           ("pool", dict(w=2, factor=4)), ("pool", dict(ldk=56)), ("pool", dict(ldvp=68)), ("pool", dict(kp=2)), ("pool", dict(v=8)),
           ("attn", dict(q=None)), ("attn", dict(o=None)), ("attn", dict(seq_kv=0)), ("attn", dict(seq_q=-1)), ("attn", dict(heads=0)),
           ("attn", dict(ldk=32)), ("attn", dict(ldo=68)), ("attn", dict(ldv=1 << 24)), ("attn", dict(k=8)),
           ("attn", dict(scale=0.0)), ("attn", dict(scale=float("inf")))]


@pytest.mark.parametrize("which,bad", REFUSED, ids=[f"{w}-{'-'.join(f'{k}={v}' for k, v in b.items())}" for w, b in REFUSED])
def test_refusals_return_negative_and_leave_the_outputs_untouched(which, bad):
    from vdpp_amd import hip
    lib = hip.load()
    src = torch.ones(64, 192, dtype=torch.float16, device=DEV)
    outs = [torch.full((64, 64), 5.0, dtype=torch.float16, device=DEV) for _ in range(2)]
    a = dict(POOL_OK if which == "pool" else ATTN_OK, **bad)
    # pointer arguments: None stays null, an integer is a byte offset into a real buffer (2 and 8: misaligned)
    ptr = lambda t, off: None if off is None else t.data_ptr() + off
    if which == "pool":
        rc = lib.sp_kv_pool_f16(ptr(src, a["k"]), ptr(src, a["v"]), a["ldk"], a["ldv"], ptr(outs[0], a["kp"]), ptr(outs[1], a["vp"]),
                                a["ldkp"], a["ldvp"], a["n_img"], a["h"], a["w"], a["c"], a["factor"], None)
    else:
        rc = lib.sp_attn_spatial_kv_f16(ptr(src, a["q"]), ptr(src, a["k"]), ptr(src, a["v"]), ptr(outs[0], a["o"]), a["ldq"], a["ldk"],
                                        a["ldv"], a["ldo"], a["batch"], a["seq_q"], a["seq_kv"], a["heads"], a["scale"], None)
    torch.cuda.synchronize()
    assert rc < 0 and hip.load().sp_last_error(), f"rc={rc}"
    assert all(bool((t == 5.0).all()) for t in outs)
