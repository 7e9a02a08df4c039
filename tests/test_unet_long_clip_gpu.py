"""Clips longer than 32 frames per UNet call: the tiny engine at 40 frames against the fp32 oracle as
``tests/test_unet_gpu.py::test_unet_forward_matches_oracle`` checks 14 frames (same comparison, its tolerance: relative L2 <=
2e-2), one sampler step at 40 frames, the routing at 14 frames left as it was, the refusal beyond 128 frames."""
import pytest
import torch

from tests.test_unet_gpu import _build, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _kinds(fn):      # (fn's result, the kinds of the ops timing table filled while it ran)
    from vdpp_amd.hip import ops
    ops.PROFILE = log = []
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.PROFILE = None
    return out, {rec[0] for rec in log}


def test_unet_forward_40_frames_matches_oracle_and_14_frames_keep_their_kernel():
    cfg, sd, ref, hip = _build()
    g = torch.Generator().manual_seed(11)
    sample = torch.randn(1, 40, 8, 16, 16, generator=g).half()        # latent (1, 4, 40, 16, 16) ++ image latents
    ctx = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half()
    ids, t = torch.tensor([[5.0, 127.0, 0.02]]).half(), 1.63777
    with torch.no_grad():
        want = ref(sample.float(), t, ctx.float(), ids.float())[0]
    (got,), kinds = _kinds(lambda: hip(sample.to(DEV), t, ctx.to(DEV), ids.to(DEV)))
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = rel_l2(got.float(), want)
    print(f"UNet forward at 40 frames: rel_l2 {err:.3e}")
    assert err <= 2e-2, f"UNet forward rel_l2={err:.3e}"
    assert "attn_temporal_long" in kinds and "attn_temporal" not in kinds
    _, short = _kinds(lambda: hip(sample[:, :14].to(DEV), t, ctx.to(DEV), ids.to(DEV)))
    assert "attn_temporal" in short and "attn_temporal_long" not in short


def test_step_at_40_frames_and_refusal_beyond_128():
    from vdpp_amd.models.svd_unet import StableVideoUNet
    from vdpp_amd.models.unet_spec import UNetConfig
    cfg = UNetConfig.tiny(64)
    model = StableVideoUNet.from_random_init(StableVideoUNet._default_timestep_schedule(25), config=cfg, device=DEV)
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half().to(DEV)
    for frames in (40, 136):
        model.set_conditioning(emb, torch.randn(1, 4, frames, 8, 8, generator=g).half().to(DEV), num_frames=frames)
        lat = (torch.randn(1, 4, frames, 8, 8, generator=g) * model.init_noise_sigma).half().to(DEV)
        if frames > 128:
            with pytest.raises(ValueError, match="window_stride"):
                model(lat, 0)
        else:
            new = model(lat, 0)
            assert new.shape == lat.shape and torch.isfinite(new).all() and not torch.equal(new, lat)
