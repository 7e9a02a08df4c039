"""``SVDUNetHIP(kv_downsample=2)``: whole-UNet parity against the fp32 oracle whose spatial self-attention pools K and V over
2 x 2 cells of the token grid the same way (fp32, no rounding), under ``peaked_state_dict`` so that the attention shows;
and the switch itself: off is the default forward, other factors are refused, on is reproducible across graph replay."""
import pytest
import torch

from oracle import svd_unet_ref as R
from tests import unet_mutants as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pool_patch(monkeypatch, h, w, factor=2, levels=4):
    """Patch the oracle's scaled_dot_product_attention: self-attention over exactly the tokens of a level whose grid
    divides by ``factor`` sees K and V averaged over factor x factor cells; everything else (temporal sequences, the
    context token, the coarsest level) passes through."""
    grids = {(h >> i) * (w >> i): (h >> i, w >> i) for i in range(levels) if (h >> i) % factor == 0 and (w >> i) % factor == 0}
    plain = R.F.scaled_dot_product_attention

    def sdpa(q, k, v, **kw):
        n = k.shape[-2]
        if n in grids and q.shape[-2] == n:
            gh, gw = grids[n]
            k, v = [t.reshape(*t.shape[:2], gh // factor, factor, gw // factor, factor, -1).mean((3, 5)).flatten(2, 3) for t in (k, v)]
        return plain(q, k, v, **kw)
    monkeypatch.setattr(R.F, "scaled_dot_product_attention", sdpa)
    return grids


@pytest.fixture(scope="module")
def net():
    cfg, _ = M.configs()
    sd = M.peaked_state_dict(cfg, M.SEED)
    return cfg, sd, M.build_oracle(sd)


@pytest.mark.parametrize("case,factor", [pytest.param(case, f, id=case if f == 2 else f"{case}-factor4") for f in (2, 4) for case in M.CASES])
def test_kv_downsample_unet_matches_pooling_oracle(net, case, factor, monkeypatch):
    """Bound: FACTOR x the fp16-storage emulation's error, both sides of it under the patch (nothing from the engine).  With
    factor 2 the patch covers three levels (down to two keys), with factor 4 the two finest (in the 2 x 3 x 16 x 24 case
    16 x 24 and 8 x 12: non-square, 24 and 6 keys); the unpatched oracle is at least 10 bounds away, so an engine that never
    pooled cannot pass.  (Oracle alone, on the CPU: 68 to 87 bounds away with factor 2, 79 to 93 with factor 4.)"""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, ref = net
    b, frames, h, w = M.CASES[case]
    assert frames not in [(h >> i) * (w >> i) for i in range(4)]           # a temporal sequence is never taken for a level
    if factor == 4 and (h % 4 or w % 4):
        pytest.skip(f"no level of a {h} x {w} latent divides by 4: nothing would be pooled")
    sample, ctx, ids = M.case_inputs(cfg, case)
    unpooled = M.run_oracle(ref, sample, ctx, ids)
    with monkeypatch.context() as mp:
        assert len(_pool_patch(mp, h, w, factor)) == (3 if factor == 2 else 2)
        want, _, noise = M.noise_and_bounds(ref, sample, ctx, ids)
    hip = SVDUNetHIP(cfg, sd, DEV, kv_downsample=factor, kv_downsample_min_tokens=1)
    got = hip(sample.to(DEV), M.TIMESTEP, ctx.to(DEV), ids.to(DEV))[0].float().cpu()
    bound, err, away = M.FACTOR * noise["final"], M.rel_l2(got, want), M.rel_l2(unpooled, want)
    print(f"kv_downsample={factor} {case}: engine vs pooling oracle {err:.3e} (bound {bound:.3e}); unpooled oracle vs pooling oracle {away:.3e}")
    assert torch.isfinite(got).all()
    assert away >= 10 * bound, f"the pooled and the unpooled oracle differ by {away:.3e} < 10 x {bound:.3e}"
    assert err <= bound, f"rel_l2={err:.3e}, bound={bound:.3e}"


def _args(cfg, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, 3, 8, 8, 16, generator=g).half().to(DEV), 0.6,
            torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half().to(DEV), torch.tensor([[5.0, 127.0, 0.02]]).half().to(DEV))


def test_kv_downsample_off_is_the_default_forward(net, monkeypatch):
    """None with the environment unset, 1, and an engine built without the argument: the same bytes; 2 gives others."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = net
    monkeypatch.delenv("VDPP_KV_DOWNSAMPLE", raising=False)
    absent, none, one = SVDUNetHIP(cfg, sd, DEV), SVDUNetHIP(cfg, sd, DEV, kv_downsample=None), SVDUNetHIP(cfg, sd, DEV, kv_downsample=1)
    assert absent.kv_downsample == none.kv_downsample == one.kv_downsample == 1
    args = _args(cfg)
    base = absent(*args)[0]
    assert torch.equal(none(*args)[0], base) and torch.equal(one(*args)[0], base)
    assert not torch.equal(SVDUNetHIP(cfg, sd, DEV, kv_downsample=2, kv_downsample_min_tokens=1)(*args)[0], base)


@pytest.mark.parametrize("factor", [3, 0, 8])
def test_kv_downsample_refuses_other_factors(net, factor):
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = net
    with pytest.raises(ValueError, match="kv_downsample"):
        SVDUNetHIP(cfg, sd, DEV, kv_downsample=factor)


def test_kv_downsample_is_bit_identical_across_calls_and_graph_replay(net):
    from vdpp_amd.models.svd_unet import StableVideoUNet
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _ = net
    hip = SVDUNetHIP(cfg, sd, DEV, kv_downsample=2, kv_downsample_min_tokens=1)
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
