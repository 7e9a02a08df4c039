"""Whole-UNet parity that can see attention: the HIP engine against the fp32 oracle under ``peaked_state_dict``
(tests/unet_mutants.py: self-attention logits of standard deviation 3 instead of 0.3, so that every softmax row has a
dominant key), judged at the final output AND at every resnet / transformer block.

Bounds: ``T = 3 x`` the error of the oracle's fp16-storage emulation (the output of every Linear / Conv / GroupNorm /
LayerNorm rounded to fp16) for the same quantity on the same inputs -- computed here from the oracle alone, never from
the engine.  Why 3: at default weights the engine's recorded error (1.2-1.4e-3) is 1.5-1.7 x the emulation's
8e-4; the rest covers the attention kernels' own roundings (Q pre-multiplied and rounded to fp16, P in fp16), which the
emulation lacks -- the pre-rounded Q alone moves the final output by 4e-4 under the recipe.
tests/test_unet_sensitivity_cpu.py shows on the CPU that every mutant of tests/unet_mutants.py moves the quantity compared
here by at least 2 T at these shapes (table: profiles/unet_sensitivity.txt).  Every test prints the measured error
beside its bound, per block (pytest -s)."""
import pytest
import torch

from tests import unet_mutants as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def net():
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    cfg, _ = M.configs()
    sd = M.peaked_state_dict(cfg, M.SEED)
    return cfg, M.build_oracle(sd), SVDUNetHIP(cfg, sd, DEV)


@pytest.mark.parametrize("case", list(M.CASES))
def test_unet_peaked_weights_match_oracle_at_every_block(net, case):
    """Final output within T, then every block's output within that block's T, then every transformer's branch
    (output - input) within its T.  Two videos: also each video's output within its own T."""
    cfg, ref, hip = net
    sample, ctx, ids = M.case_inputs(cfg, case)
    want, blocks, noise = M.noise_and_bounds(ref, sample, ctx, ids)
    with M.capture_engine(hip) as seen:
        got = hip(sample.to(DEV), M.TIMESTEP, ctx.to(DEV), ids.to(DEV))[0]
    torch.cuda.synchronize()
    got = got.float().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    M.assert_same_blocks(seen, blocks)

    err = M.rel_l2(got, want)
    print(f"\n{case}: final output rel-L2 {err:.2e}  (T = {M.FACTOR * noise['final']:.2e})")
    print(f"  {'block':<32s} {'output':>9s} {'T':>9s}   {'branch':>9s} {'T':>9s}")
    late_out, late_branch = {}, {}
    for i, (e, o) in enumerate(zip(seen, blocks)):
        e_out, t_out = M.rel_l2(e.y, o.y), M.FACTOR * noise["out"][i]
        line = f"  {i:2d} {o.name:<29s} {e_out:9.2e} {t_out:9.2e}"
        if e_out > t_out:
            late_out[o.name] = f"{e_out:.2e} > {t_out:.2e}"
        if o.kind == "xf":
            e_br, t_br = M.rel_l2(e.branch.cpu(), o.branch), M.FACTOR * noise["branch"][i]
            line += f"   {e_br:9.2e} {t_br:9.2e}"
            if e_br > t_br:
                late_branch[o.name] = f"{e_br:.2e} > {t_br:.2e}"
        print(line)
    assert err <= M.FACTOR * noise["final"], f"final output rel_l2={err:.3e}, T={M.FACTOR * noise['final']:.3e}"
    for v in range(want.shape[0]) if want.shape[0] > 1 else ():
        e_v, t_v = M.rel_l2(got[v], want[v]), M.FACTOR * M.rel_l2(noise["emu"][v], want[v])
        print(f"  video {v}: {e_v:.2e}  (T = {t_v:.2e})")
        assert e_v <= t_v, f"video {v}: rel_l2={e_v:.3e}, T={t_v:.3e}"
    assert not late_out, f"block outputs beyond their bound: {late_out}"
    assert not late_branch, f"transformer branches beyond their bound: {late_branch}"


def test_step_with_guidance_under_peaked_weights_matches_oracle_step(net):
    """One step of ``StableVideoUNet.forward`` with guidance 3.0 (two UNet passes, per-frame guidance mix, Euler update)
    against ``oracle/svd_step_ref.py`` driving the fp32 oracle.  T for the updated latent is derived as above: 3 x the error
    of the same step with the fp16-storage emulation as its UNet, input and eps rows in fp16 and the new latent rounded
    to fp16.  Step 18 of 25 (sigma 0.68 -> 0.34), where the update is a fifth of the latent and half of the emulation's
    2.9e-4 comes from the eps rows (the rest is the fp16 rounding of the new latent); the update's own error is printed."""
    from oracle.svd_step_ref import svd_step
    from vdpp_amd.models.svd_unet import StableVideoUNet

    cfg, ref, hip = net
    model = StableVideoUNet(unet=hip, timesteps=StableVideoUNet._default_timestep_schedule(25))
    frames, h, w, step, guidance = 4, 8, 16, 18, 3.0
    g = torch.Generator().manual_seed(21)
    emb = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half()
    img = torch.randn(1, 4, frames, h, w, generator=g).half()
    lat = (torch.randn(1, 4, frames, h, w, generator=g) * float(model.sigmas[step] + 1)).half()
    model.set_conditioning(emb.to(DEV), img.to(DEV), guidance_scale=guidance, num_frames=frames)
    got = model(lat.to(DEV), step).float().cpu()
    model.clear_conditioning()

    def stored16(sample, timestep, encoder_hidden_states, added_time_ids, return_dict=False):
        return (ref(sample.half().float(), timestep, encoder_hidden_states, added_time_ids)[0].half().float(),)

    kw = dict(sigmas=model.sigmas, timesteps=model.scheduler_timesteps, image_embeddings=emb.float(), image_latents=img.float(),
              added_time_ids=torch.tensor([[5.0, 127.0, 0.02]]).half().float(), guidance_scale=guidance, dtype=torch.float32)
    with torch.no_grad():
        want = svd_step(ref, lat.float(), step, **kw)
        with M.fp16_storage(ref):
            emu = svd_step(stored16, lat.float(), step, **kw).half().float()
    err, t = M.rel_l2(got, want), M.FACTOR * M.rel_l2(emu, want)
    upd = M.rel_l2(got - lat.float(), want - lat.float())
    t_upd = M.FACTOR * M.rel_l2(emu - lat.float(), want - lat.float())
    print(f"\nstep {step}, guidance {guidance}: new latent rel-L2 {err:.2e} (T = {t:.2e}); update {upd:.2e} (its T: {t_upd:.2e}); "
          f"update / latent = {float((want - lat.float()).norm() / want.norm()):.2f}")
    assert torch.isfinite(got).all()
    assert err <= t, f"updated latent rel_l2={err:.3e}, T={t:.3e}"
