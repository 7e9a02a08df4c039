"""sp_conv_up2x_f16 (``ops.gemm(..., up2x_phases=True)``): a nearest x2 upsample + 3x3 convolution as four 2x2 phase
convolutions, against fp32 torch on the fp16-rounded inputs -- with the ORIGINAL 3x3 weights (project tolerances: relative L2
2e-3, max 1e-2; the one extra fp16 rounding of the folded weights is 2e-4 of it) and with the folded fp16 weights the kernel
really multiplies with (same tolerances; what is left is the fp16 rounding of the output)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from vdpp_amd.hip import ops
    return ops


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def check(out, ref, l2=2e-3, mx=1e-2):
    out, ref = out.float().cpu(), ref.float().cpu()
    assert torch.isfinite(out).all()
    e = rel_l2(out, ref)
    m = float((out - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    print(f"rel_l2={e:.3e} max_rel={m:.3e}")
    assert e <= l2 and m <= mx, f"rel_l2={e:.3e} max_rel={m:.3e}"


def ref_nine_tap(x, w, bias):
    """x [B][H][W][C], w [N][C][3][3] fp32 on any device -> rows [B*2H*2W][N]: nine shifted matrix products (no convolution
    library between the test and its reference; checked against F.conv2d in the first case)."""
    b, hh, ww, c = x.shape
    up = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    upp = F.pad(up, (0, 0, 1, 1, 1, 1))
    out = bias.to(x.device).float().expand(b * 4 * hh * ww, -1).clone()
    for ky in range(3):
        for kx in range(3):
            out += upp[:, ky:ky + 2 * hh, kx:kx + 2 * ww].reshape(-1, c) @ w[:, :, ky, kx].t()
    return out


def ref_phases(x, pack, bias, cin):
    """The same from the kernel's own operand: pack [4][N][4*Cpad] fp16 (as include/svdpipe.h states the sum)."""
    b, hh, ww, c = x.shape
    n, cp = pack.shape[1], pack.shape[2] // 4
    wf = pack.float().reshape(4, n, 2, 2, cp)[..., :cin]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.empty(b, 2 * hh, 2 * ww, n, dtype=torch.float32, device=x.device)
    for py in range(2):
        for px in range(2):
            acc = bias.to(x.device).float().expand(b * hh * ww, -1).clone()
            for ty in range(2):
                for tx in range(2):
                    acc += xp[:, py + ty:py + ty + hh, px + tx:px + tx + ww].reshape(-1, c) @ wf[2 * py + px, :, ty, tx].t()
            out[:, py::2, px::2] = acc.reshape(b, hh, ww, n)
    return out.reshape(-1, n)


def run_case(n_img, hh, ww, cin, n, *, seed, ref_dev="cpu", cross_check=False):
    ops = _ops()
    from vdpp_amd.models import weights as W
    g = torch.Generator().manual_seed(seed)
    cp = W.round_up(cin, 64)
    x = torch.randn(n_img, hh, ww, cin, generator=g).half()
    w = (torch.randn(n, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).half()
    bias = torch.randn(n, generator=g)
    pack = W.pack_conv3x3_up2x(w, cp, n)
    a = torch.zeros(n_img * hh * ww, cp, dtype=torch.float16)
    a[:, :cin] = x.reshape(-1, cin)
    m = n_img * 4 * hh * ww
    out = torch.full((m, n), float("nan"), dtype=torch.float16, device=DEV)
    ops.gemm(a.to(DEV), pack.to(DEV), out, m=m, n=n, cin=cp, mode=ops.A_CONV3X3, conv=(n_img, hh, ww, 2 * hh, 2 * ww, 1, 1),
             bias=bias.to(DEV), up2x_phases=True)
    assert ops.load().sp_gemm_last_kernel().decode() == f"gemm_pp_kernel<256, {320 if n % 320 == 0 else 256}, 8192>"
    want = ref_nine_tap(x.float().to(ref_dev), w.float().to(ref_dev), bias)
    if cross_check:
        conv = F.conv2d(F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), w.float(), bias, padding=1)
        assert rel_l2(want, conv.permute(0, 2, 3, 1).reshape(m, n)) <= 1e-6
    check(out, want)
    check(out, ref_phases(x.float().to(ref_dev), pack.to(ref_dev), bias, cin))
    return out


@pytest.mark.parametrize("n", [320, 256])
def test_ragged_tiles_that_straddle_images(n):
    """297 rows per phase: two tiles per phase, the second ragged, image borders inside both; 96 channels padded to 128."""
    run_case(3, 9, 11, 96, n, seed=n, cross_check=True)


@pytest.mark.parametrize("hh,ww", [(1, 5), (5, 1)])
def test_images_that_are_all_border(hh, ww):
    run_case(2, hh, ww, 64, 256, seed=hh * 10 + ww)


def test_benchmarks_smallest_layer_one_round_of_workgroups():
    """28 frames of 9 x 16, 1280 -> 1280 channels: 4 phases x 16 row tiles (the last of each ragged: 4,032 rows) x 4 column
    tiles = 256 workgroups.  The reference runs on the GPU as fp32 matrix products."""
    torch.backends.cuda.matmul.allow_tf32 = False
    run_case(28, 9, 16, 1280, 1280, seed=5, ref_dev=DEV)


@pytest.mark.parametrize("hh,ww", [(16, 16), (16, 32)])
def test_column_slice_output_and_column_sums_for_the_next_groupnorm(hh, ww):
    """2 frames of 16 x 16 (one tile per frame and phase) and of 16 x 32 (two: the kernel's frame / tile-in-frame split of the
    column sums' tile index), 64 -> 320 channels, the output a column slice of a wider buffer whose slack is NaN and stays NaN.
    With gn_part: GroupNorm(+SiLU) from the column sums against torch on the stored output (tolerances of
    test_groupnorm_statistics_from_the_producing_contraction), per frame and over all rows.  Then the tile order: with
    weights on a grid of 1/64 the fold is exact in fp16, the phase and the nine-tap call compute the same sums in another
    order, and the per-frame (mean, rstd) the fold kernel derives from either call's column sums agree to 1e-5 relative
    (the bias puts every group's mean near 3, far from zero) -- they would not if a frame's tiles stood anywhere else."""
    ops = _ops()
    from vdpp_amd.models import weights as W
    n_img, cin, n, slack = 2, 64, 320, 64
    m = n_img * 4 * hh * ww
    conv = (n_img, hh, ww, 2 * hh, 2 * ww, 1, 1)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n_img, hh, ww, cin, generator=g).half()
    w = (torch.randn(n, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).half()
    bias = torch.randn(n, generator=g) + 3.0
    gamma, beta = 1.0 + 0.3 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    a = x.reshape(-1, cin).to(DEV)

    def phases(weights, gn):
        buf = torch.full((m, slack + n + slack), float("nan"), dtype=torch.float16, device=DEV)
        out = buf[:, slack:slack + n]
        part = torch.full((m // 256, 2, n, 2), float("nan"), dtype=torch.float32, device=DEV) if gn else None
        ops.gemm(a, W.pack_conv3x3_up2x(weights, cin, n).to(DEV), out, m=m, n=n, cin=cin, mode=ops.A_CONV3X3, conv=conv,
                 bias=bias.to(DEV), ldd=buf.stride(0), gn_part=part, up2x_phases=True)
        assert torch.isnan(buf[:, :slack]).all() and torch.isnan(buf[:, slack + n:]).all()
        return out, part

    def norm_stats(out, part, ni, nr):
        y = torch.empty((m, n), dtype=torch.float16, device=DEV)
        stats = torch.full((ni * 32 * 2,), float("nan"), dtype=torch.float32, device=DEV)
        ops.groupnorm_tile_sums(out, part, gamma.to(DEV), beta.to(DEV), y, instances=ni, rows=nr, c=n, groups=32, eps=1e-6,
                                silu=True, stats=stats, ldx=out.stride(0))
        return y, stats.double().cpu().reshape(ni, 32, 2)

    out, part = phases(w, True)
    plain, _ = phases(w, False)
    assert torch.equal(out, plain), "asking for the column sums changed the output"
    check(out, ref_nine_tap(x.float(), w.float(), bias))
    assert torch.isfinite(part).all()
    for ni, nr in ((n_img, m // n_img), (1, m)):
        y, _ = norm_stats(out, part, ni, nr)
        ref = F.silu(F.group_norm(out.double().cpu().reshape(ni, nr, n).permute(0, 2, 1), 32, gamma.double(), beta.double(),
                                  eps=1e-6)).permute(0, 2, 1).reshape(m, n).float()
        check(y, ref, l2=2e-3, mx=2e-2)

    wg = (torch.randint(-32, 33, (n, cin, 3, 3), generator=g) / 64.0).half()       # folds of up to four stay exact in fp16
    assert torch.equal(W.fold_conv3x3_up2x(wg.float()).half().float(), W.fold_conv3x3_up2x(wg.float()))
    out_p, part_p = phases(wg, True)
    out_9 = torch.empty((m, n), dtype=torch.float16, device=DEV)
    part_9 = torch.full((m // 256, 2, n, 2), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm(a, W.pack_conv3x3(wg, cin, n).to(DEV), out_9, m=m, n=n, cin=cin, mode=ops.A_CONV3X3, conv=conv, bias=bias.to(DEV),
             gn_part=part_9)
    check(out_p, out_9.float(), l2=1e-4, mx=2e-3)       # the same sums in another order: fp16 roundings that fall the other way
    _, st_p = norm_stats(out_p, part_p, n_img, m // n_img)
    _, st_9 = norm_stats(out_9, part_9, n_img, m // n_img)
    mean_p, rstd_p, mean_9, rstd_9 = st_p[..., 0], st_p[..., 1], st_9[..., 0], st_9[..., 1]
    d_mean = float(((mean_p - mean_9).abs() / mean_9.abs()).max())
    d_rstd = float(((rstd_p - rstd_9).abs() / rstd_9).max())
    print(f"per-frame statistics, phases against nine taps: mean {d_mean:.2e} rstd {d_rstd:.2e}")
    assert d_mean <= 1e-5 and d_rstd <= 1e-5


def test_tiny_unet_forward_with_and_without_phases():
    """UNetConfig.tiny(256) at 32 x 32: 4x4 -> 8x8 runs as phases without column sums, 8x8 -> 16x16 keeps the nine taps (too
    small to pay for the statistics pass), 16x16 -> 32x32 runs as phases and leaves the sums.  On against off: 2e-3."""
    ops = _ops()
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict
    cfg = UNetConfig.tiny(256)
    eng = SVDUNetHIP(cfg, random_state_dict(cfg, seed=3, dtype=torch.float16), DEV)
    assert eng.upsample_phases
    g = torch.Generator().manual_seed(3)
    sample = torch.randn(1, 2, 8, 32, 32, generator=g).half()
    ctx = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half()
    ids = torch.tensor([[5.0, 127.0, 0.02]])
    ops.PROFILE = log = []
    try:
        on = eng(sample, 0.6, ctx, ids)[0].float().cpu()
        kernels_on = [t[5][-1] for t in log if t[0] == "gemm"]
        del log[:]
        eng.upsample_phases = False
        off = eng(sample, 0.6, ctx, ids)[0].float().cpu()
        kernels_off = [t[5][-1] for t in log if t[0] == "gemm"]
    finally:
        ops.PROFILE = None
    assert sum("8192>" in k for k in kernels_on) == 2 and not any("8192>" in k for k in kernels_off)
    assert len(kernels_on) == len(kernels_off)
    e = rel_l2(on, off)
    print(f"tiny UNet, phases on against off: rel_l2={e:.3e}")
    assert torch.isfinite(on).all() and e <= 2e-3
