"""``SVDUNetHIP(fp8_ff=True)``: whole-UNet parity against the fp32 oracle with the GEGLU first projections fake-quantised the
same way, and the switch itself: off changes nothing, on is reproducible across graph replay and row chunks."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 3.0          # engine vs emulation, as tests/test_edge_peaked_gpu.py


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _fq(t):           # per-row amax/448 scale, e4m3 round trip
    s = t.abs().amax(-1, keepdim=True) / 448.0
    s = torch.where(s > 0, s, torch.ones_like(s))
    return (t / s).to(torch.float8_e4m3fn).float() * s


def _fake_quantise(ref, half_inputs):
    """Oracle hooks: a GEGLU projection sees its LayerNorm's un-affine output (``half_inputs``: of the fp16-rounded input)
    fake-quantised per row against its gamma-folded weights fake-quantised per output channel."""
    handles = []
    for blk in (m for m in ref.modules() if hasattr(m, "norm3")):
        for norm, ff in [(blk.norm3, blk.ff)] + ([(blk.norm_in, blk.ff_in)] if hasattr(blk, "norm_in") else []):
            def keep(mod, inp, out):
                x = inp[0].half().float() if half_inputs else inp[0]
                mod.y = F.layer_norm(x, mod.normalized_shape, None, None, mod.eps)
            def proj(mod, inp, out, norm=norm):
                return _fq(norm.y) @ _fq(mod.weight * norm.weight[None, :]).t() + (mod.weight @ norm.bias + mod.bias)
            handles += [norm.register_forward_hook(keep), ff.net[0].proj.register_forward_hook(proj)]
    return handles


def _build(seed, **kw):
    from oracle.svd_unet_ref import SVDUNetConfig, SVDUNetRef
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict
    cfg = UNetConfig.tiny(64)
    sd = random_state_dict(cfg, seed=seed, dtype=torch.float16)
    ref = SVDUNetRef(SVDUNetConfig.tiny(64)).eval()
    ref.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return cfg, sd, ref, SVDUNetHIP(cfg, sd, DEV, **kw)


@pytest.mark.parametrize("b,frames,h,w", [(1, 3, 16, 24), (2, 4, 8, 16)])
def test_fp8_ff_unet_matches_fake_quantised_oracle(b, frames, h, w):
    """fp16 storage moves some activations across an e4m3 rounding boundary, so the bound is measured on the reference alone:
    the fake-quantised oracle against itself with the FF1 inputs rounded to fp16 first; the engine is held to FACTOR x that."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, ref, hip8 = _build(3, fp8_ff=True)
    g = torch.Generator().manual_seed(11 + b)
    sample = torch.randn(b, frames, 8, h, w, generator=g).half()
    ctx = torch.randn(b, 1, cfg.cross_attention_dim, generator=g).half()        # per-video conditioning
    ids = torch.tensor([[5.0, 127.0, 0.02], [9.0, 60.0, 0.1]])[:b].half()
    t = 1.63777
    with torch.no_grad():
        outs = []
        for half in (None, False, True):              # unquantised (information only), fake-quantised, ... on fp16 inputs
            hooks = [] if half is None else _fake_quantise(ref, half_inputs=half)
            outs.append(ref(sample.float(), t, ctx.float(), ids.float())[0])
            [hd.remove() for hd in hooks]
    plain, want, floor = outs[0], outs[1], rel_l2(outs[2], outs[1])
    args = (sample.to(DEV), t, ctx.to(DEV), ids.to(DEV))
    got8 = hip8(*args, per_video=b > 1)[0].float()
    got16 = SVDUNetHIP(cfg, sd, DEV)(*args, per_video=b > 1)[0].float()
    assert torch.isfinite(got8).all() and not torch.equal(got8, got16)
    e8 = rel_l2(got8, want)
    print(f"fp8_ff b={b} frames={frames} {h}x{w}: floor {floor:.3e}, engine vs fake-quantised oracle {e8:.3e} (bound {FACTOR * floor:.3e}); "
          f"vs unquantised oracle: fp8_ff {rel_l2(got8, plain):.3e}, fp16 {rel_l2(got16, plain):.3e}")
    assert e8 <= FACTOR * floor


def test_fp8_ff_with_kv_downsample_matches_the_doubly_patched_oracle(monkeypatch):
    """``fp8_ff=True, kv_downsample=2`` in one engine: ``_ff1``'s e4m3 bytes and ``_self_attn``'s pooled K / V live in the same
    stream scratch pool in the same forward.  Reference: the oracle under BOTH patches (fake-quantised first projections,
    K and V pooled over 2 x 2 cells on the three levels whose grid divides).  Bound as in the test above: measured on that
    oracle alone (FF1 inputs rounded to fp16 first, against not), times FACTOR; nothing from the engine enters it.  The
    result differs from either single-switch engine's, and is the same bytes on a second call and with the feed-forward
    pairs in row chunks (1,152 rows x 256 hidden in five chunks at level 0)."""
    from tests.test_unet_kv_downsample_gpu import _pool_patch
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    b, frames, h, w = 1, 3, 16, 24
    kv = dict(kv_downsample=2, kv_downsample_min_tokens=1)
    cfg, sd, ref, both = _build(3, fp8_ff=True, **kv)
    g = torch.Generator().manual_seed(11 + b)
    sample = torch.randn(b, frames, 8, h, w, generator=g).half()
    ctx = torch.randn(b, 1, cfg.cross_attention_dim, generator=g).half()
    ids = torch.tensor([[5.0, 127.0, 0.02]]).half()
    t = 1.63777
    with torch.no_grad(), monkeypatch.context() as mp:
        assert sorted(_pool_patch(mp, h, w).values()) == [(4, 6), (8, 12), (16, 24)]
        outs = []
        for half in (False, True):
            hooks = _fake_quantise(ref, half_inputs=half)
            outs.append(ref(sample.float(), t, ctx.float(), ids.float())[0])
            [hd.remove() for hd in hooks]
    want, floor = outs[0], rel_l2(outs[1], outs[0])
    args = (sample.to(DEV), t, ctx.to(DEV), ids.to(DEV))
    got = both(*args)[0].clone()
    assert torch.isfinite(got).all()
    assert not torch.equal(got, SVDUNetHIP(cfg, sd, DEV, fp8_ff=True)(*args)[0]), "the same bytes as fp8_ff alone: nothing was pooled"
    assert not torch.equal(got, SVDUNetHIP(cfg, sd, DEV, **kv)(*args)[0]), "the same bytes as kv_downsample alone: no fp8 projection"
    assert torch.equal(both(*args)[0], got), "second call"
    both.FF_CHUNK_BYTES, both.FF_CHUNK_ROUND = 1 << 17, 256
    try:
        assert torch.equal(both(*args)[0], got), "feed-forward pairs in row chunks"
    finally:
        both.FF_CHUNK_BYTES, both.FF_CHUNK_ROUND = 0, None
    err = rel_l2(got.float(), want)
    print(f"fp8_ff + kv_downsample=2 b={b} frames={frames} {h}x{w}: floor {floor:.3e}, engine vs doubly patched oracle {err:.3e} "
          f"(bound {FACTOR * floor:.3e})")
    assert err <= FACTOR * floor


def test_fp8_ff_off_is_the_default_forward():
    """Flag absent (environment unset) and flag False: two engines from one state dict, the same bytes, no e4m3 pack."""
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, sd, _, absent = _build(7)
    off = SVDUNetHIP(cfg, sd, DEV, fp8_ff=False)
    assert not absent.fp8_ff and not off.fp8_ff and not hasattr(off.mid[1]["s_ff1"], "w8")
    g = torch.Generator().manual_seed(5)
    args = (torch.randn(1, 3, 8, 8, 16, generator=g).half().to(DEV), 0.6,
            torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half().to(DEV), torch.tensor([[5.0, 127.0, 0.02]]).half().to(DEV))
    assert torch.equal(absent(*args)[0], off(*args)[0])


@pytest.mark.parametrize("how", ["graph", "chunks"])
def test_fp8_ff_is_bit_identical_across(how):
    from vdpp_amd.models.svd_unet import StableVideoUNet
    cfg, sd, _, hip = _build(19, fp8_ff=True)
    g = torch.Generator().manual_seed(6)
    frames, h, w = 3, 16, 16
    emb = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half().to(DEV)
    img = torch.randn(1, 4, frames, h, w, generator=g).half().to(DEV)
    ts = StableVideoUNet._default_timestep_schedule(25)
    eager, other = StableVideoUNet(unet=hip, timesteps=ts), StableVideoUNet(unet=hip, timesteps=ts)
    for m in (eager, other):
        m.set_conditioning(emb, img, num_frames=frames)
    for trial in range(3):                       # graph: the first call captures, the later ones replay with new data
        lat = (torch.randn(1, 4, frames, h, w, generator=g) * 100).half().to(DEV)
        want = eager(lat, 3)
        if how == "graph":
            other.enable_graphs()
        else:
            hip.FF_CHUNK_BYTES, hip.FF_CHUNK_ROUND = 1 << 17, 256      # level 0: 768 rows x 256 hidden in three chunks
        try:
            got = other(lat, 3)
        finally:
            hip.FF_CHUNK_BYTES, hip.FF_CHUNK_ROUND = 0, None
        assert torch.equal(got, want), f"{how}, trial {trial}"
    other.enable_graphs(False)
