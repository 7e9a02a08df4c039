"""Bit-exact parity of sp_gemm_f16 (and sp_conv_up2x_f16) on integer-grid operands.

Every operand is a small non-zero integer (tests/gemm_model.py: ``make_exact_tensors``, the value ladder RUNGS), every product
and every partial sum an integer below 2^24: fp32 addition of those is exact and associative, so the result does not depend on
tile shape, split-K, ring depth or MFMA order, and the stored fp16 must equal the integer reference BIT FOR BIT.  One dropped,
doubled or misplaced term is a non-zero integer difference (tests/test_exact_patterns_cpu.py plants seven such bugs and shows
that the tolerance of the descriptor fuzz lets two of them pass).  Per draw, on every forced route:

* buffers, guards, NaN slack, the repeat and the workspace overrun check are the descriptor fuzz's own (``launch``);
* ``d`` as int16 equals the reference as int16;
* ``gn_part`` equals the integer sums exactly (fp32-side values without residuals, stored values with: the same numbers here);
* ``ln_out`` keeps the tolerance of its dedicated test (a mean and a 1 / sqrt are not integers).

GEGLU and the Euler tail are not exact (``gemm_model.exact_eligible``) and stay on the fuzz's tolerances.  A failing draw
prints the first differing (row, column) and got - want: in integer units that names the missing term.  Replay:
``tools/fuzz_gemm.py --descriptor ROUTE BM INDEX --exact``."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_model as M  # noqa: E402
import test_gemm_descriptor_fuzz_gpu as fz  # noqa: E402

DEV = "cuda"


def first_difference(got, want):
    """'' or a description of the first element (row-major) where two [m][n] tensors differ."""
    bad = (got.double() != want.double()).nonzero()
    if not len(bad):
        return ""
    r, c = int(bad[0, 0]), int(bad[0, 1])
    rows = sorted(set(bad[:, 0].tolist()))
    return (f"{len(bad)} of {got.numel()} values differ in {len(rows)} rows (first rows {rows[:4]}); first at (row {r}, column {c}): "
            f"got {float(got[r, c])} want {float(want[r, c])}, got - want = {float(got[r, c]) - float(want[r, c])}")


def run_exact(d, lib, zero_page):
    """One eligible draw at its rung: returns (rung, kernel)."""
    rung, bufs, views, ref = M.exact_case(d)
    d, got, stored, sizes, kernel, what = fz.launch(d, lib, zero_page, bufs, views)
    what["rung"] = rung
    want = ref["d"].half()
    assert torch.equal(want.double(), ref["d"])
    have = stored.half()
    if not torch.equal(have.view(torch.int16), want.view(torch.int16)):
        e = M.errors(stored, ref["d"])
        raise AssertionError(f"d is not the integer result ({kernel}): {first_difference(have, want)}; by the fuzz's measure "
                             f"global rel_l2={e[0]:.3e} worst 64x64 block={e[1]:.3e}: {what}")
    if d["ln_out"]:
        fz.check_ln_out(d, got, stored, kernel, what)
    if d["gn_part"]:
        m, n = d["m"], d["n"]
        have = got["gn_part"][:sizes["gn_part"]].reshape(m // 256 * 2, n, 2)
        sums = M.half_tile_sums(ref["d"]).reshape(m // 256 * 2, n, 2)
        for j, name in enumerate(("sums", "sums of squares")):
            assert torch.equal(sums[..., j].float().double(), sums[..., j])
            diff = first_difference(have[..., j], sums[..., j].float())
            assert not diff, f"gn_part {name} (row = 128-row half tile) are not the integer sums ({kernel}): {diff}: {what}"
    return rung, kernel


@pytest.mark.parametrize("route,bm", M.ROUTES)
def test_gemm_exact(route, bm):
    from vdpp_amd.hip import ops
    lib = ops.load()
    zero_page = ops.zero_page(torch.device(DEV))
    draws = M.exact_draws(route, bm)
    kernels, rungs = [], []
    with (ops.gemm_route(3, bm=256, bn=192) if bm == -192 else ops.gemm_route(route, bm=bm)):
        for i, d in enumerate(draws):
            try:
                rung, kernel = run_exact(d, lib, zero_page)
            except AssertionError as err:
                raise AssertionError(f"route ({route}, {bm}) exact draw {i}: {err}") from None
            kernels.append(kernel)
            rungs.append(rung)
    own = [k for k in kernels if k.startswith(fz.family(route, bm)) and (route != 4 or "splitk_reduce_kernel" in k)]
    print(f"exact route ({route}, {bm}): {len(draws)} draws, rungs {rungs}, its own family ran {len(own)} times, "
          f"{len(set(kernels))} different kernels")
    assert len(own) >= 5, f"route ({route}, {bm}): its own family ran {len(own)} times: {sorted(set(kernels))}"


@pytest.mark.parametrize("route,bm", [(0, 0), (1, 0), (2, 256), (2, 128), (4, 0)])
@pytest.mark.parametrize("case", sorted(M.EXACT_FIXED))
def test_gemm_exact_edge_geometries(case, route, bm):
    from vdpp_amd.hip import ops
    d = M.exact_fixed(case)
    if route == 4:
        d.update(workspace=M.FAKE["workspace"], workspace_bytes=64)
    with ops.gemm_route(route, bm=bm):
        run_exact(d, ops.load(), ops.zero_page(torch.device(DEV)))


@pytest.mark.parametrize("n_img,hh,ww,cin,n", [(2, 5, 3, 64, 256), (3, 9, 11, 128, 320)])
def test_conv_up2x_phases_exact(n_img, hh, ww, cin, n):
    """sp_conv_up2x_f16: weights on the 1/64 grid fold exactly in fp16 (sums of up to four of them), activations are integers
    in [-3, 3]: the four folded phases must equal the nine-tap integer reference bit for bit, in a column slice of a NaN
    buffer between guard rows.  (Units of 1/64: |sum| <= 9 * cin * 3 * 32 + bias < 2^24.)"""
    from vdpp_amd.hip import ops
    from vdpp_amd.models import weights as W
    g = torch.Generator().manual_seed(1000 + n)
    x = M._ints(g, (n_img, hh, ww, cin), 3)
    w = M._ints(g, (n, cin, 3, 3), 8) / 64.0
    bias = M._ints(g, (n,), 8)
    assert torch.equal(W.fold_conv3x3_up2x(w).half().float(), W.fold_conv3x3_up2x(w))
    d = M.blank()
    d.update(mode=M.CONV3X3, n_img=n_img, hin=hh, win=ww, hout=2 * hh, wout=2 * ww, stride=1, upsample2x=1, m=n_img * 4 * hh * ww,
             n=n, cin=cin, bias=1)
    # the model's weight layout is [n][tap][cin] as gather_rows concatenates the taps
    views = {"a": x.reshape(-1, cin).half(), "w": w.permute(0, 2, 3, 1).reshape(1, n, 9 * cin).half(), "bias": bias}
    want = M.reference(d, views)["d"]
    assert torch.equal(want.half().double(), want) and 9 * cin * 3 * 8 + 8 * 64 < M.EXACT_LIMIT
    m, slack, guard = d["m"], 24, 3
    buf = torch.full((m + 2 * guard, slack + n + slack), float("nan"), dtype=torch.float16, device=DEV)
    out = buf[guard:guard + m, slack:slack + n]
    ops.gemm(x.reshape(-1, cin).half().to(DEV), W.pack_conv3x3_up2x(w.half(), cin, n).to(DEV), out, m=m, n=n, cin=cin,
             mode=ops.A_CONV3X3, conv=(n_img, hh, ww, 2 * hh, 2 * ww, 1, 1), bias=bias.to(DEV), ldd=buf.stride(0), up2x_phases=True)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.isnan(got[:guard]).all() and torch.isnan(got[guard + m:]).all(), "guard rows written"
    assert torch.isnan(got[:, :slack]).all() and torch.isnan(got[:, slack + n:]).all(), "slack columns written"
    have = got[guard:guard + m, slack:slack + n].contiguous()
    assert torch.equal(have.view(torch.int16), want.half().view(torch.int16)), first_difference(have, want.half())
