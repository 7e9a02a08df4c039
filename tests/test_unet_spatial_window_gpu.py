"""``SVDUNetHIP(spatial_window=(1, 1))``: whole-UNet parity against the fp32 oracle whose spatial self-attention carries the
boolean mask of the sliding tile window (8 x 8 token tiles, the window shifted inwards at the borders), under
``peaked_state_dict`` so that the attention shows; and the switch itself: off is the default forward, a window that
covers every grid is full attention, bad values are refused, on is reproducible across graph replay."""
import pytest
import torch

from oracle import svd_unet_ref as R
from tests import unet_mutants as M
from tests.test_attn_window_gpu import window_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _window_patch(monkeypatch, h, w, window, levels=4):
    """Patch the oracle's scaled_dot_product_attention: self-attention over exactly the tokens of a level whose grid
    divides by 8 gets the window's boolean ``attn_mask``; everything else (temporal sequences, the context token, the
    coarser levels) passes through."""
    masks = {(h >> i) * (w >> i): window_mask(h >> i, w >> i, *window) for i in range(levels) if (h >> i) % 8 == 0 and (w >> i) % 8 == 0}
    plain = R.F.scaled_dot_product_attention

    def sdpa(q, k, v, **kw):
        n = k.shape[-2]
        if n in masks and q.shape[-2] == n:
            kw = dict(kw, attn_mask=masks[n])
        return plain(q, k, v, **kw)
    monkeypatch.setattr(R.F, "scaled_dot_product_attention", sdpa)
    return masks


@pytest.fixture(scope="module")
def net():
    cfg, _ = M.configs()
    sd = M.peaked_state_dict(cfg, M.SEED)
    return cfg, sd, M.build_oracle(sd)


# (the 8 x 8 case is left out: level 0 is one tile there, (1, 1) is full attention and nothing would show)
@pytest.mark.parametrize("case", [c for c in M.CASES if M.CASES[c][2:] != (8, 8)])
def test_spatial_window_unet_matches_masked_oracle(net, case, monkeypatch):
    """Bound: FACTOR x the fp16-storage emulation's error, both sides of it under the patch (nothing from the engine).  Level 0
    is 1 x 2 and 2 x 3 tiles in the two cases and the only level whose grid divides by 8; the unpatched oracle is at least
    10 bounds away, so an engine that ran full attention cannot pass."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, ref = net
    b, frames, h, w = M.CASES[case]
    assert frames not in [(h >> i) * (w >> i) for i in range(4)]           # a temporal sequence is never taken for a level
    sample, ctx, ids = M.case_inputs(cfg, case)
    full = M.run_oracle(ref, sample, ctx, ids)
    with monkeypatch.context() as mp:
        assert list(_window_patch(mp, h, w, (1, 1))) == [h * w]
        want, _, noise = M.noise_and_bounds(ref, sample, ctx, ids)
    hip = SVDUNetHIP(cfg, sd, DEV, spatial_window=(1, 1), spatial_window_min_tokens=1)
    got = hip(sample.to(DEV), M.TIMESTEP, ctx.to(DEV), ids.to(DEV))[0].float().cpu()
    bound, err, away = M.FACTOR * noise["final"], M.rel_l2(got, want), M.rel_l2(full, want)
    print(f"spatial_window=(1, 1) {case}: engine vs masked oracle {err:.3e} (bound {bound:.3e}); full oracle vs masked oracle {away:.3e}")
    assert torch.isfinite(got).all()
    assert away >= 10 * bound, f"the windowed and the full oracle differ by {away:.3e} < 10 x {bound:.3e}"
    assert err <= bound, f"rel_l2={err:.3e}, bound={bound:.3e}"


def test_window_that_covers_every_grid_is_full_attention(net):
    """(3, 3) on the 16 x 24 latent (2 x 3 tiles): against the UNPATCHED oracle, within the same kind of bound."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, ref = net
    sample, ctx, ids = M.case_inputs(cfg, "2x3x16x24")
    want, _, noise = M.noise_and_bounds(ref, sample, ctx, ids)
    hip = SVDUNetHIP(cfg, sd, DEV, spatial_window=(3, 3), spatial_window_min_tokens=1)
    got = hip(sample.to(DEV), M.TIMESTEP, ctx.to(DEV), ids.to(DEV))[0].float().cpu()
    bound, err = M.FACTOR * noise["final"], M.rel_l2(got, want)
    print(f"spatial_window=(3, 3) on 2 x 3 tiles: engine vs full oracle {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"rel_l2={err:.3e}, bound={bound:.3e}"


def test_spatial_window_off_is_the_default_forward(net, monkeypatch):
    """None with the environment unset and an engine built without the argument: the same bytes; (1, 1) gives others."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = net
    monkeypatch.delenv("VDPP_SPATIAL_WINDOW", raising=False)
    absent, none = SVDUNetHIP(cfg, sd, DEV), SVDUNetHIP(cfg, sd, DEV, spatial_window=None)
    assert absent.spatial_window is None and none.spatial_window is None
    g = torch.Generator().manual_seed(5)
    args = (torch.randn(1, 3, 8, 8, 16, generator=g).half().to(DEV), 0.6,
            torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half().to(DEV), torch.tensor([[5.0, 127.0, 0.02]]).half().to(DEV))
    base = absent(*args)[0]
    assert torch.equal(none(*args)[0], base)
    assert not torch.equal(SVDUNetHIP(cfg, sd, DEV, spatial_window=(1, 1), spatial_window_min_tokens=1)(*args)[0], base)


@pytest.mark.parametrize("kw", [dict(spatial_window=(2, 3)), dict(spatial_window=(3, 0)), dict(spatial_window=(3,)), dict(spatial_window=(True, 3)),
                                dict(spatial_window=(3.0, 3)), dict(spatial_window=5), dict(spatial_window=(3, 3), kv_downsample=2)],
                         ids=lambda kw: "-".join(f"{v}" for v in kw.values()))
def test_spatial_window_refuses_bad_values_and_kv_downsample(net, kw):
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = net
    with pytest.raises(ValueError, match="spatial_window"):
        SVDUNetHIP(cfg, sd, DEV, **kw)


def test_spatial_window_is_bit_identical_across_calls_and_graph_replay(net):
    from vdpp_amd.models.svd_unet import StableVideoUNet
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = net
    hip = SVDUNetHIP(cfg, sd, DEV, spatial_window=(1, 1), spatial_window_min_tokens=1)
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
