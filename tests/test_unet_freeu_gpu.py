"""``SVDUNetHIP(freeu=(b1, b2, s1, s2))``: whole-UNet parity against the fp32 oracle whose up resnets see their concatenated
input rewritten by the torch.fft statement of FreeU (a forward pre-hook, fp32), under ``peaked_state_dict``; the switch
is reproducible across calls and graph replay, and refuses values that are not finite and positive."""
import functools

import pytest
import torch

from tests import unet_mutants as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
FREEU = (1.5, 1.6, 0.2, 0.4)
CASE = "2x3x16x24"           # two videos of different scale and conditioning; levels 16 x 24 down to 2 x 3


def _freeu(cl, b, s, version, module, args):
    x = args[0].clone()
    factor = b
    if version == 2:
        m = x[:, :cl].mean(1, keepdim=True)
        lo, hi = m.amin((2, 3), keepdim=True), m.amax((2, 3), keepdim=True)
        factor = (b - 1) * (m - lo) / (hi - lo) + 1
    x[:, :cl // 2] *= factor
    h, w = x.shape[-2:]
    mask = torch.ones(h, w)
    mask[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1] = s
    spec = torch.fft.fftshift(torch.fft.fftn(x[:, cl:], dim=(-2, -1)), dim=(-2, -1)) * mask
    x[:, cl:] = torch.fft.ifftn(torch.fft.ifftshift(spec, dim=(-2, -1)), dim=(-2, -1)).real
    return (x,) + tuple(args[1:])


def _hook(ref, version):
    """Pre-hooks on the up resnets whose running tensor has 4*c0 (b1, s1) or 2*c0 (b2, s2) channels -> their handles."""
    c0, run = ref.cfg.block_out_channels[0], ref.cfg.block_out_channels[-1]
    pairs, handles = {4 * c0: (FREEU[0], FREEU[2]), 2 * c0: (FREEU[1], FREEU[3])}, []
    for blk in ref.up_blocks:
        for res in blk.resnets:
            if run in pairs:
                handles.append(res.register_forward_pre_hook(functools.partial(_freeu, run, *pairs[run], version)))
            run = res.spatial_res_block.conv1.out_channels
    assert len(handles) == 10
    return handles


@pytest.fixture(scope="module")
def net():
    cfg, _ = M.configs()
    sd = M.peaked_state_dict(cfg, M.SEED)
    return cfg, sd, M.build_oracle(sd)


@pytest.mark.parametrize("version", [1, 2])
def test_freeu_unet_matches_hooked_oracle(net, version):
    """Bound: FACTOR x the fp16-storage emulation's error, both sides of it under the hooks (nothing from the engine); the
    oracle without hooks is at least 10 bounds away, so an engine that ignored the option cannot pass.  (Oracle alone, on
    the CPU: 66 bounds away at version 1, 54 at version 2.)"""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, ref = net
    sample, ctx, ids = M.case_inputs(cfg, CASE)
    plain = M.run_oracle(ref, sample, ctx, ids)
    handles = _hook(ref, version)
    try:
        want, _, noise = M.noise_and_bounds(ref, sample, ctx, ids)
    finally:
        for hd in handles:
            hd.remove()
    hip = SVDUNetHIP(cfg, sd, DEV, freeu=FREEU, freeu_version=version)
    got = hip(sample.to(DEV), M.TIMESTEP, ctx.to(DEV), ids.to(DEV))[0].float().cpu()
    bound, err, away = M.FACTOR * noise["final"], M.rel_l2(got, want), M.rel_l2(plain, want)
    print(f"freeu v{version} {CASE}: engine vs hooked oracle {err:.3e} (bound {bound:.3e}); plain oracle vs hooked oracle {away:.3e}")
    assert torch.isfinite(got).all()
    assert away >= 10 * bound, f"the oracle with and without FreeU differ by {away:.3e} < 10 x {bound:.3e}"
    assert err <= bound, f"rel_l2={err:.3e}, bound={bound:.3e}"


def test_freeu_is_bit_identical_across_calls_and_graph_replay(net):
    from vdpp_amd.models.svd_unet import StableVideoUNet
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = net
    hip = SVDUNetHIP(cfg, sd, DEV, freeu=FREEU)
    g = torch.Generator().manual_seed(6)
    frames, h, w = 3, 16, 16
    emb = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half().to(DEV)
    img = torch.randn(1, 4, frames, h, w, generator=g).half().to(DEV)
    ts = StableVideoUNet._default_timestep_schedule(25)
    eager, graphed = StableVideoUNet(unet=hip, timesteps=ts), StableVideoUNet(unet=hip, timesteps=ts)
    for m in (eager, graphed):
        m.set_conditioning(emb, img, num_frames=frames)
    graphed.enable_graphs()
    for trial in range(3):                       # the first call captures, the later ones replay with new data
        lat = (torch.randn(1, 4, frames, h, w, generator=g) * 100).half().to(DEV)
        want = eager(lat, 3)
        assert torch.equal(eager(lat, 3), want), f"second eager call, trial {trial}"
        assert torch.equal(graphed(lat, 3), want), f"graph, trial {trial}"
    graphed.enable_graphs(False)


@pytest.mark.parametrize("freeu,version", [((1.5, 1.6, 0.2), 2), ((1.5, 1.6, 0.0, 0.4), 2), ((1.5, float("inf"), 0.2, 0.4), 2),
                                           ((1.5, 1.6, float("nan"), 0.4), 1), ((-1.5, 1.6, 0.2, 0.4), 1), (FREEU, 3)])
def test_freeu_refuses_other_values(net, freeu, version):
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = net
    with pytest.raises(ValueError, match="freeu"):
        SVDUNetHIP(cfg, sd, DEV, freeu=freeu, freeu_version=version)
