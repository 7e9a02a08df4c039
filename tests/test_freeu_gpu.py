"""csrc/freeu.hip through the C ABI: ``sp_freeu_f16`` against the torch.fft statement of FreeU's skip filter and the
version-1 / version-2 backbone scale, both in fp64 on the CPU from the same fp16 inputs (independent of the kernel's
projection form); the patterns that admit no tolerance; the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
# (n_img, h, w, c_left, c_right, extra pitch): Nyquist == frequency -1; odd sizes and three images; a ragged last slab;
# several token chunks per image; the longest fold (36 chunks)
CASES = [(1, 2, 2, 16, 8, 0), (3, 3, 5, 16, 8, 8), (2, 9, 16, 32, 72, 0), (2, 36, 64, 128, 64, 16), (1, 72, 128, 16, 8, 0)]


def _call(lib, cat, ld, n, h, w, cl, cr, b, s, version, ws):
    rc = lib.sp_freeu_f16(cat.data_ptr(), ld, n, h, w, cl, cr, b, s, version, ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc


def _run(data, case, b, s, version):
    """``data`` fp16 [n*h*w][c_left + c_right] on the CPU -> (result, the whole buffer before, after): the rows sit in a
    NaN-filled buffer with 8 guard rows on either side and the extra pitch."""
    from vdpp_amd import hip
    n, h, w, cl, cr, extra = case
    lib, ld = hip.load(), cl + cr + extra
    full = torch.full((n * h * w + 16, ld), float("nan"), dtype=torch.float16, device=DEV)
    full[8:-8, :cl + cr] = data.to(DEV)
    before = full.clone()
    ws = torch.empty(lib.sp_freeu_ws_bytes(n, h, w, cl, cr), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0 and _call(lib, full[8:-8], ld, n, h, w, cl, cr, b, s, version, ws) == 0, hip.last_error()
    return full[8:-8, :cl + cr].cpu(), before.cpu().view(torch.int16), full.cpu().view(torch.int16)


def _data(case, seed=0):
    """Images of different scales (x1, x2, x3), so that a sum, a minimum or a maximum that mixed images would show."""
    n, h, w, cl, cr, _ = case
    x = torch.randn(n, h * w, cl + cr, generator=torch.Generator().manual_seed(seed + h * w)) * torch.arange(1, n + 1).view(n, 1, 1)
    return x.reshape(n * h * w, cl + cr).half()


def _ulp16(v):
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 10)


def _reference(data, case, b, s, version):
    """fp64 -> (left reference, its bound, right reference, its bound), each [n][C][h][w]; the bounds: see the parity test."""
    n, h, w, cl, cr, _ = case
    x = data.double().view(n, h, w, cl + cr).permute(0, 3, 1, 2)
    left, skip = x[:, :cl // 2], x[:, cl:]
    if version == 1:
        factor, dm = torch.full((n, 1, h, w), b, dtype=torch.float64), 0.0
    else:
        m = x[:, :cl].mean(1, keepdim=True)
        lo, hi = m.amin((2, 3), keepdim=True), m.amax((2, 3), keepdim=True)
        factor = (b - 1) * (m - lo) / (hi - lo) + 1
        e_m = 32 * U * x[:, :cl].abs().mean(1, keepdim=True).amax((2, 3), keepdim=True)
        dm = 4 * e_m / (hi - lo) + 4 * U
    want_l = left * factor
    bound_l = _ulp16(want_l) + left.abs() * abs(b - 1) * dm + 4 * U * want_l.abs()
    mask = torch.ones(h, w, dtype=torch.float64)
    mask[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1] = s
    spec = torch.fft.fftshift(torch.fft.fftn(skip, dim=(-2, -1)), dim=(-2, -1)) * mask
    want_r = torch.fft.ifftn(torch.fft.ifftshift(spec, dim=(-2, -1)), dim=(-2, -1)).real
    bound_r = _ulp16(want_r) + 96 * U * (7 * abs(s - 1) * skip.abs().mean((2, 3), keepdim=True) + want_r.abs())
    return want_l, bound_l, want_r, bound_r


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_freeu_matches_the_fft_statement(case, version):
    """Bound per element: one fp16 ulp of the fp64 result, plus
    * skip filter: 96 * 2^-24 of the terms.  A coefficient is sum_m phi(m) x[m] with |phi| <= 1: a thread adds at most 8
      terms here (chunks of 256 rows over 32 row lanes), then 3 xor levels, 3 wave adds and at most 36 chunk adds = 50
      roundings, and phi itself is off by at most 16 * 2^-24 (sincospif of an argument rounded in [-1, 1], the addition
      formulas); seven coefficients times |s - 1|/(h w) meet the mean |x| of the (image, channel), and the final
      x + sum rounds in fp32 a few more times (the term in |result|): 50 + 16 + 8 <= 96.
    * backbone scale, version 2: |x| (b - 1) * (4 e_m/(hi - lo) + 4 * 2^-24), e_m = 32 * 2^-24 * mean_c |x| at the image's
      worst pixel (a row sum: at most 24 sequential adds and 6 xor levels, one division), which m, lo and hi each carry;
      version 1 and the product itself: 4 * 2^-24 of the result.
    Columns outside the two ranges, pad columns and guard rows keep their bytes; a second call gives the same bytes."""
    n, h, w, cl, cr, _ = case
    b, s = 1.4, 0.3
    data = _data(case)
    got, before, after = _run(data, case, b, s, version)
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[8:-8, :cl // 2] = False
    keep[8:-8, cl:cl + cr] = False
    assert torch.equal(after[keep], before[keep]), "bytes outside [0, c_left/2) and [c_left, c_left + c_right) changed"
    assert torch.equal(_run(data, case, b, s, version)[2], after), "two calls, two results"
    want_l, bound_l, want_r, bound_r = _reference(data, case, b, s, version)
    g = got.double().view(n, h, w, cl + cr).permute(0, 3, 1, 2)
    err_l, err_r = (g[:, :cl // 2] - want_l).abs(), (g[:, cl:] - want_r).abs()
    print(f"freeu v{version} {case}: backbone max err {float(err_l.max()):.3e} ({float((err_l / bound_l).max()):.3f} of its bound), "
          f"skip max err {float(err_r.max()):.3e} ({float((err_r / bound_r).max()):.3f} of its bound)")
    assert bool((err_l <= bound_l).all()) and bool((err_r <= bound_r).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_freeu_exact_patterns(case):
    n, h, w, cl, cr, _ = case
    data = _data(case, seed=1)
    for version in (1, 2):                                        # b = s = 1: the input's bytes
        _, before, after = _run(data, case, 1.0, 1.0, version)
        assert torch.equal(after, before)
    # every pixel of an image the same row: the skip is constant per channel, s = 2^-1 gives exactly s * x; the channel
    # mean is the same at every pixel (hi == lo), version 2 leaves the backbone as it is
    const = data.view(n, h * w, -1)[:, :1].expand(n, h * w, cl + cr).reshape(n * h * w, cl + cr)
    got, _, _ = _run(const, case, 1.5, 0.5, 2)
    assert torch.equal(got[:, cl:], (const[:, cl:].float() * 0.5).half()) and torch.equal(got[:, :cl], const[:, :cl])
    if h % 2 == 0 and w % 2 == 0 and h > 2 and w > 2:             # +-1 checkerboard: frequency (h/2, w/2), outside the block
        y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        board = data.clone()
        board[:, cl:] = (1.0 - 2.0 * ((x + y) % 2)).reshape(1, h * w, 1).expand(n, h * w, cr).reshape(n * h * w, cr).half()
        assert torch.equal(_run(board, case, 1.0, 0.25, 1)[0], board)


OK = dict(cat=0, ld=32, n=1, h=4, w=4, cl=16, cr=8, b=1.2, s=0.5, version=2, ws=0, short=0)
REFUSED = [dict(cat=None), dict(ws=None), dict(n=0), dict(h=-4), dict(h=1), dict(w=1), dict(cl=24), dict(cl=0), dict(cr=12),
           dict(ld=16), dict(ld=28), dict(cat=8), dict(version=3), dict(version=0), dict(b=0.0), dict(b=float("inf")),
           dict(s=float("nan")), dict(s=-0.5), dict(short=4)]


@pytest.mark.parametrize("bad", REFUSED, ids=["-".join(f"{k}={v}" for k, v in b.items()) for b in REFUSED])
def test_freeu_refusals_leave_the_buffer_untouched(bad):
    from vdpp_amd import hip
    lib, a = hip.load(), dict(OK, **bad)
    buf = torch.full((16, 32), 5.0, dtype=torch.float16, device=DEV)
    ws = torch.zeros(lib.sp_freeu_ws_bytes(1, 4, 4, 16, 8), dtype=torch.uint8, device=DEV)
    ptr = lambda t, off: None if off is None else t.data_ptr() + off      # None stays null, an integer is a byte offset
    rc = lib.sp_freeu_f16(ptr(buf, a["cat"]), a["ld"], a["n"], a["h"], a["w"], a["cl"], a["cr"], a["b"], a["s"], a["version"],
                          ptr(ws, a["ws"]), ws.numel() - a["short"], None)
    torch.cuda.synchronize()
    assert rc < 0 and "sp_freeu_f16" in hip.last_error(), f"rc={rc}"
    assert bool((buf == 5.0).all()) and bool((ws == 0).all())
