"""The fp8 feed-forward kernels (csrc/gemm_f8.hip) against fp64 torch on the same e4m3 bytes and scales."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4M3 = torch.float8_e4m3fn


def _ops():
    from vdpp_amd.hip import ops
    return ops


_dec = lambda b: b.view(E4M3).double()         # e4m3 bytes -> fp64


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("n", [128, 384])
@pytest.mark.parametrize("m", [1, 257])
@pytest.mark.parametrize("k", [64, 320, 1280])
def test_gemm_f8_plain_is_exact_on_integers(k, m, n, res):
    """A, W in {-1, 0, 1}, scales in {1/2, 1}, integer bias and residual: every partial sum is a small multiple of 1/4, so
    fp32 summation is exact in any order and d must EQUAL the fp64 reference, which is its own fp16 rounding.  One k-step,
    an odd count of k-steps, the full depth; a row tail inside the first tile and behind a whole one; half a column tile."""
    ops = _ops()
    g = torch.Generator().manual_seed(1000 * k + 10 * m + n + res)
    code = torch.tensor([0xB8, 0x00, 0x38], dtype=torch.uint8)           # -1, 0, 1
    a8, w8 = code[torch.randint(0, 3, (m, k), generator=g)], code[torch.randint(0, 3, (n, k), generator=g)]
    sa, sw = 0.5 * torch.randint(1, 3, (m,), generator=g).float(), 0.5 * torch.randint(1, 3, (n,), generator=g).float()
    bias = torch.randint(-8, 9, (n,), generator=g).float()
    r1 = torch.randint(-4, 5, (m, n), generator=g).half() if res else None
    ref = sa.double()[:, None] * sw.double()[None, :] * (_dec(a8) @ _dec(w8).t()) + bias.double()
    if res:
        ref = ref + 2.0 * r1.double()
    assert torch.equal(ref.half().double(), ref), "the reference is not exactly representable in fp16"
    ldd = n + 8                                                          # slack columns and guard rows stay NaN
    d = torch.full((m + 2, ldd), float("nan"), dtype=torch.float16, device=DEV)
    ops.gemm_f8(a8.to(DEV), sa.to(DEV), w8.to(DEV), sw.to(DEV), bias.to(DEV), d[1:m + 1, :n], m=m, n=n, k=k,
                res1=r1.to(DEV) if res else None, r1scale=2.0, ldd=ldd)
    assert ops.load().sp_gemm_last_kernel() == b"gemm_f8_kernel<256, 256, 0>"
    d = d.cpu()
    assert torch.equal(d[1:m + 1, :n].view(torch.int16), ref.half().view(torch.int16))
    assert torch.isnan(d[0]).all() and torch.isnan(d[m + 1]).all() and torch.isnan(d[:, n:]).all()


@pytest.mark.parametrize("k", [320, 1280])
def test_gemm_f8_geglu_gaussian(k):
    """Gaussian operands, erf-gelu in fp64; the tolerance of the fp16 GEGLU contraction test (tests/test_kernels_gpu.py: rel-L2
    2e-3, max 1e-2 of max|ref|).  The weights are packed by models/weights.py, so the interleave is under test too."""
    ops = _ops()
    from vdpp_amd.models import weights as W
    m, n = 257, 384
    g = torch.Generator().manual_seed(k)
    a, w, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / math.sqrt(k), torch.randn(n, generator=g)
    sa = a.abs().amax(1) / 448.0
    a8 = (a / sa[:, None]).to(E4M3).view(torch.uint8)
    w8, sw = W.pack_linear_f8(w, geglu=False)
    w8i, swi = W.pack_linear_f8(w, geglu=True)
    _, bi = W.interleave_geglu(w, b)
    y = sa.double()[:, None] * sw.double()[None, :] * (_dec(a8) @ _dec(w8).t()) + b.double()
    ref = y[:, :n // 2] * F.gelu(y[:, n // 2:])
    out = torch.empty(m, n // 2, dtype=torch.float16, device=DEV)
    ops.gemm_f8(a8.to(DEV), sa.to(DEV), w8i.to(DEV), swi.to(DEV), bi.to(DEV), out, m=m, n=n, k=k, geglu=True)
    out = out.double().cpu()
    assert torch.isfinite(out).all()
    l2, mx = float((out - ref).norm() / ref.norm()), float((out - ref).abs().max() / ref.abs().max())
    print(f"gemm_f8 geglu k={k}: rel_l2={l2:.3e} max_rel={mx:.3e}")
    assert l2 <= 2e-3 and mx <= 1e-2


@pytest.mark.parametrize("c,rows", [(c, r) for c in (320, 640, 1280) for r in (1, 5, 67)] + [(320, 8200), (640, 4100), (1280, 2050)])
def test_ln_quant_f8(c, rows):
    """Few rows (one row per wave) and just past the row counts from which 16 / 8 / 4 rows share a wave.  Strided x; row 0 carries a single 1,000x spike, row 1 is constant (amax = 0: zeros, sa = 1).  y in fp64 from the
    statistics the kernel reads.  Seeds: the fp32 CPU evaluation of the reference agrees with the fp64 one in >= 99.9 % of
    the bytes for every case."""
    ops = _ops()
    g = torch.Generator().manual_seed(c + rows)
    x = torch.randn(rows, c + 8, generator=g).half()
    x[0, 7] = 1000.0
    if rows > 1:
        x[1] = 0.5
    xd = x.to(DEV)
    st = torch.empty(rows, 2, device=DEV)
    ops.ln_stats(xd[:, :c].contiguous(), st, rows=rows, c=c)
    q = torch.full((rows, c + 16), 0x7F, dtype=torch.uint8, device=DEV)
    sa = torch.empty(rows, device=DEV)
    ops.ln_quant_f8(xd[:, :c], st, q[:, :c], sa, rows=rows, c=c, ldx=c + 8, ldq=c + 16)
    st, q, sa = st.double().cpu(), q.cpu(), sa.cpu()
    assert (q[:, c:] == 0x7F).all(), "bytes behind the row were written"
    q = q[:, :c]
    y = (x[:, :c].double() - st[:, :1]) * st[:, 1:]
    amax = y.abs().amax(1)
    want_sa = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).float()
    ulps = (sa.double() - want_sa.double()).abs() / torch.from_numpy(np.spacing(want_sa.numpy())).double()
    assert float(ulps.max()) <= 2.0, f"sa is {float(ulps.max())} ulp off"
    if rows > 1:
        assert float(sa[1]) == 1.0 and (q[1] == 0).all()
    assert ((q & 0x7F) != 0x7F).all(), "a NaN code"
    err = (_dec(q) * sa.double()[:, None] - y).abs()
    assert (err <= 2.0 ** -4 * y.abs() + sa.double()[:, None] * 2.0 ** -10).all(), "more than half an e4m3 step"
    want_q = (y / sa.double()[:, None]).float().to(E4M3).view(torch.uint8)
    same = float((q == want_q).double().mean())
    print(f"ln_quant_f8 c={c} rows={rows}: {100 * same:.3f} % of the bytes equal the fp64 reference's")
    assert same >= 0.99


@pytest.mark.parametrize("bad,field", [(dict(k=96), "k=96"), (dict(n=64), "n=64"), (dict(m=0), "m=0"), (dict(off=1), "a8")])
def test_gemm_f8_refuses(bad, field):
    ops = _ops()
    m, n, k, off = (bad.get(key, default) for key, default in (("m", 4), ("n", 128), ("k", 128), ("off", 0)))
    a8 = torch.zeros(8 * 128 + 16, dtype=torch.uint8, device=DEV)[off:]
    w8 = torch.zeros(128 * 128, dtype=torch.uint8, device=DEV)
    f = torch.zeros(128, device=DEV)
    with pytest.raises(ops.HipKernelError, match=field):
        ops.gemm_f8(a8, f, w8, f, f, torch.empty(4, 128, dtype=torch.float16, device=DEV), m=m, n=n, k=k, lda=128, ldd=128)
