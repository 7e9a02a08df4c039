"""Per-video conditioning on the GPU: videos of one UNet call with their own timestep, added-time ids (fps, motion bucket,
noise augmentation) and guidance scale, against the fp32 oracle of each video alone; the shared path unchanged bit for
bit; the full-width model at the benchmark shape; per-sample conditioning through interleaved lanes, eager and graphed."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _build(c=64, seed=3):
    from oracle.svd_unet_ref import SVDUNetConfig, SVDUNetRef
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict

    cfg = UNetConfig.tiny(c)
    sd = random_state_dict(cfg, seed=seed, dtype=torch.float16)
    ref = SVDUNetRef(SVDUNetConfig.tiny(c)).eval()
    ref.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return cfg, sd, ref, SVDUNetHIP(cfg, sd, DEV)


def _ids(fps, mb, na):
    return torch.tensor([[f - 1, m, a] for f, m, a in zip(fps, mb, na)]).half()


@pytest.mark.parametrize("b", [2, 3])
def test_unet_call_per_video_matches_oracle(b):
    """``__call__(per_video=True)`` with a timestep, an id row and a context of its own per video: each video against the
    fp32 oracle's batch-1 forward with its own values, 2e-2 relative L2 (as the shared-conditioning batch test)."""
    cfg, sd, ref, hip = _build(seed=41)
    frames, h, w = 4, 8, 16
    g = torch.Generator().manual_seed(200 + b)
    sample = torch.randn(b, frames, 8, h, w, generator=g).half()
    ctx = torch.randn(b, 1, cfg.cross_attention_dim, generator=g).half()
    ids = _ids([6, 12, 3][:b], [127, 20, 255][:b], [0.02, 0.3, 0.0][:b])
    t = torch.tensor([0.91, -0.35, 1.7][:b])
    got = hip(sample.to(DEV), t, ctx.to(DEV), ids.to(DEV), per_video=True)[0].float().cpu()
    for i in range(b):
        with torch.no_grad():
            want = ref(sample[i:i + 1].float(), float(t[i]), ctx[i:i + 1].float(), ids[i:i + 1].float())[0]
        err = rel_l2(got[i:i + 1], want)
        assert err <= 2e-2, f"video {i} of {b}: rel_l2={err:.3e}"


def test_id_rows_are_per_video():
    """Two videos with the same latent and context: swapping their id rows swaps their outputs; a batch whose second row
    differs changes video 1 and leaves video 0 as in the shared-ids call."""
    cfg, sd, ref, hip = _build(seed=43)
    g = torch.Generator().manual_seed(7)
    one = torch.randn(1, 4, 8, 8, 16, generator=g).half()
    sample = one.repeat(2, 1, 1, 1, 1).to(DEV)
    ctx = torch.randn(1, 1, cfg.cross_attention_dim, generator=g).half().repeat(2, 1, 1).to(DEV)
    ids = _ids([6, 20], [127, 10], [0.02, 0.5]).to(DEV)
    out = hip(sample, 0.6, ctx, ids, per_video=True)[0].float()
    swapped = hip(sample, 0.6, ctx, ids.flip(0), per_video=True)[0].float()
    assert rel_l2(out[0], out[1]) > 1e-2, "the two id rows gave the same output"
    assert rel_l2(swapped[0], out[1]) <= 1e-3 and rel_l2(swapped[1], out[0]) <= 1e-3
    shared = hip(sample, 0.6, ctx, ids[:1].repeat(2, 1))[0].float()
    assert rel_l2(out[0], shared[0]) <= 1e-3
    assert rel_l2(out[1], shared[1]) > 1e-2
    with pytest.raises(ValueError, match="added_time_ids"):
        hip(sample, 0.6, ctx, ids)                            # without per_video=True: refused as before


def test_uniform_values_take_the_shared_path_bit_for_bit():
    from vdpp_amd.models.svd_unet import StableVideoUNet

    cfg, sd, ref, hip = _build(seed=45)
    g = torch.Generator().manual_seed(9)
    sample = torch.randn(2, 4, 8, 8, 16, generator=g).half().to(DEV)
    ctx = torch.randn(2, 1, cfg.cross_attention_dim, generator=g).half().to(DEV)
    same = _ids([6, 6], [127, 127], [0.02, 0.02]).to(DEV)
    assert torch.equal(hip(sample, torch.tensor([0.4, 0.4]), ctx, same, per_video=True)[0], hip(sample, 0.4, ctx, same)[0])

    model = StableVideoUNet(unet=hip, timesteps=StableVideoUNet._default_timestep_schedule(25))
    frames = 4
    emb = torch.randn(2, 1, cfg.cross_attention_dim, generator=g).half().to(DEV)
    img = torch.randn(2, 4, frames, 8, 16, generator=g).half().to(DEV)
    lat = (torch.randn(2, 4, frames, 8, 16, generator=g) * 20).half().to(DEV)
    for guidance in (None, 3.0):
        model.set_conditioning(emb, img, fps=6, motion_bucket_id=127, noise_aug_strength=0.02, guidance_scale=guidance,
                               num_frames=frames)
        want = model(lat, 3)
        c = model.prepare_conditioning(emb, img, fps=[6, 6], motion_bucket_id=[127, 127], noise_aug_strength=[0.02, 0.02],
                                       guidance_scale=None if guidance is None else [guidance, guidance], num_frames=frames)
        assert c.added_ids32.dim() == 1 and c.guidance_ld == 0
        assert torch.equal(model(lat, 3, conditioning=c), want)


@pytest.mark.parametrize("batched_cfg", [False, True])
def test_steps_with_per_video_settings_match_oracle_step(batched_cfg):
    """Per-video (fps, motion bucket, noise aug) and guidance [3.0, 1.8], sequential passes (Euler tail in conv_out's
    epilogue) and batched CFG (sp_euler_step_rows_f16): each video's new latent against the oracle step of that video
    alone, 2e-2 relative L2.  The epilogue tail is bit-identical to the stand-alone step with ld_guidance = F."""
    from oracle.svd_step_ref import svd_step
    from vdpp_amd.hip import ops
    from vdpp_amd.models.svd_unet import StableVideoUNet

    cfg, sd, ref, hip = _build(seed=47)
    model = StableVideoUNet(unet=hip, timesteps=StableVideoUNet._default_timestep_schedule(25), batched_cfg=batched_cfg)
    frames, h, w = 4, 8, 16
    g = torch.Generator().manual_seed(13)
    emb = torch.randn(2, 1, cfg.cross_attention_dim, generator=g).half()
    img = torch.randn(2, 4, frames, h, w, generator=g).half()
    fps, mb, na, gs = [6, 10], [127, 30], [0.02, 0.2], [3.0, 1.8]
    c = model.prepare_conditioning(emb.to(DEV), img.to(DEV), fps=fps, motion_bucket_id=mb, noise_aug_strength=na,
                                   guidance_scale=gs, num_frames=frames)
    assert c.added_ids32.shape == (2, 3) and c.guidance32.shape == (2, frames) and c.guidance_ld == frames
    for step in (0, 12):
        lat = (torch.randn(2, 4, frames, h, w, generator=g) * float(model.sigmas[step] + 1)).half()
        got = model(lat.to(DEV), step, conditioning=c).float().cpu()
        for i in range(2):
            with torch.no_grad():
                want = svd_step(ref, lat[i:i + 1].float(), step, sigmas=model.sigmas, timesteps=model.scheduler_timesteps,
                                image_embeddings=emb[i:i + 1].float(), image_latents=img[i:i + 1].float(),
                                added_time_ids=_ids(fps[i:i + 1], mb[i:i + 1], na[i:i + 1]).float(), guidance_scale=gs[i],
                                dtype=torch.float32)
            err = rel_l2(got[i:i + 1], want)
            assert err <= 2e-2, f"step {step} video {i}: rel_l2={err:.3e}"
    if not batched_cfg:
        lat = (torch.randn(2, 4, frames, h, w, generator=g) * 30).half().to(DEV)
        step = 5
        fused = model(lat, step, conditioning=c)
        sigma, sigma_next = model._sigma_host[step], model._sigma_host[step + 1]
        in_scale = 1.0 / (sigma * sigma + 1.0) ** 0.5
        eps_u = model._unet_pass(lat, c.uncond_image_latents, c.uncond_embeddings, in_scale, step, added_ids32=c.added_ids32)
        eps_c = model._unet_pass(lat, c.image_latents, c.image_embeddings, in_scale, step, added_ids32=c.added_ids32)
        want = torch.empty_like(lat)
        ops.euler_step(lat, eps_c, eps_u, c.guidance32, want, ld_eps=eps_c.shape[1], sigma=sigma, sigma_next=sigma_next,
                       b=2, frames=frames, h=h, w=w, ld_guidance=frames)
        assert torch.equal(fused, want)
        shared = torch.empty_like(lat)                         # (and the rows really are used: row 0 for both differs)
        ops.euler_step(lat, eps_c, eps_u, c.guidance32[0].contiguous(), shared, ld_eps=eps_c.shape[1], sigma=sigma,
                       sigma_next=sigma_next, b=2, frames=frames, h=h, w=w)
        assert torch.equal(shared[0], want[0]) and not torch.equal(shared[1], want[1])
    with pytest.raises(ValueError, match="mix"):
        model.prepare_conditioning(emb.to(DEV), img.to(DEV), guidance_scale=[3.0, 1.0], num_frames=frames)
    with pytest.raises(ValueError, match="motion_bucket_id"):
        model.prepare_conditioning(emb.to(DEV), img.to(DEV), motion_bucket_id=[127, 30, 5], num_frames=frames)
    with pytest.raises(ValueError, match="guidance_scale"):
        model.prepare_conditioning(emb.to(DEV), img.to(DEV), guidance_scale=[3.0], num_frames=frames)


@pytest.fixture(scope="module")
def full_model():
    from vdpp_amd.models.svd_unet import StableVideoUNet
    return StableVideoUNet.from_random_init(StableVideoUNet._default_timestep_schedule(25), seed=0, device=DEV)


def test_benchmark_shape_per_video_step_equals_single_video_steps(full_model):
    """(2,4,14,72,128) on the full-width model: a step whose two videos have their own (fps, motion bucket, noise aug) --
    every resnet's time-embedding row picked per video at the 9,216 / 2,304 / 576 / 144-token levels, split-K included --
    equals each video's batch-1 step on the update it applies (2e-3, as the shared-conditioning pair test), and runs on
    exactly the contraction kernels of the shared-ids pair."""
    from vdpp_amd.hip import ops

    model, frames = full_model, 14
    g = torch.Generator().manual_seed(frames)
    emb = torch.randn(2, 1, 1024, generator=g).half().to(DEV)
    img = torch.randn(2, 4, frames, 72, 128, generator=g).half().to(DEV)
    step = 2
    lat = (torch.randn(2, 4, frames, 72, 128, generator=g) * float(model.sigmas[step])).half().to(DEV)
    fps, mb, na = [6, 14], [127, 30], [0.02, 0.25]
    c = model.prepare_conditioning(emb, img, fps=fps, motion_bucket_id=mb, noise_aug_strength=na, num_frames=frames)

    def kernels(cond):
        ops.PROFILE = []
        try:
            out = model(lat, step, conditioning=cond)
            torch.cuda.synchronize()
            return out, [rec[5] for rec in ops.PROFILE if rec[0] == "gemm"]
        finally:
            ops.PROFILE = None

    pair, routes = kernels(c)
    _, shared_routes = kernels(model.prepare_conditioning(emb, img, num_frames=frames))
    assert routes == shared_routes, "per-video time-embedding rows changed a contraction's kernel"
    assert torch.isfinite(pair).all() and torch.equal(pair, model(lat, step, conditioning=c))
    upd_pair = (pair.float() - lat.float()).cpu()
    for i in range(2):
        one = model.prepare_conditioning(emb[i:i + 1], img[i:i + 1], fps=fps[i], motion_bucket_id=mb[i],
                                         noise_aug_strength=na[i], num_frames=frames)
        single = model(lat[i:i + 1].contiguous(), step, conditioning=one)
        err = rel_l2(upd_pair[i:i + 1], (single.float() - lat[i:i + 1].float()).cpu())
        print(f"video {i}: per-video pair vs single step, rel-L2 of the update {err:.3e}")
        assert err <= 2e-3, f"video {i}: rel_l2={err:.3e}"


@pytest.mark.parametrize("per_video_batch", [False, True])
def test_lanes_and_graphs_with_per_sample_conditioning(per_video_batch):
    """concurrent_samples = 2 on one GPU, eager and with HIP graphs (capture pass + replay pass), every sample with its
    own conditioning through the supplier -- batch-1 samples, or micro-batch-2 samples with mixed per-video settings --
    bit-identical to each sample run alone under set_conditioning; one graph per (lane, step)."""
    from vdpp_amd.models.svd_unet import StableVideoUNet
    from vdpp_amd.pipeline import LatentSpec, PipelineConfig, PipelineStage

    cfg, sd, ref, hip = _build(seed=49)
    steps, n_samples, frames, h, w = 3, 4, 3, 8, 16
    b = 2 if per_video_batch else 1
    ts = StableVideoUNet._default_timestep_schedule(steps)
    alone, eager, graphed = (StableVideoUNet(unet=hip, timesteps=ts) for _ in range(3))
    graphed.enable_graphs()
    torch.manual_seed(17)
    shape = torch.Size((b, 4, frames, h, w))
    xs = [(torch.randn(shape) * 15 * (i + 1)).half().to(DEV) for i in range(n_samples)]
    embs = [torch.randn(b, 1, cfg.cross_attention_dim).half().to(DEV) for _ in range(n_samples)]
    imgs = [torch.randn(shape).half().to(DEV) for _ in range(n_samples)]

    def settings(i):
        if per_video_batch:
            return dict(fps=[6, 8 + i], motion_bucket_id=[127, 20 * i], noise_aug_strength=[0.02, 0.1],
                        guidance_scale=[3.0, 1.5 + 0.25 * i], num_frames=frames)
        return dict(fps=6 + i, motion_bucket_id=40 * i, noise_aug_strength=0.02, guidance_scale=2.0 + i, num_frames=frames)

    want = []
    for i in range(n_samples):
        alone.set_conditioning(embs[i], imgs[i], **settings(i))
        lat = xs[i]
        for s in range(steps):
            lat = alone(lat, s)
        want.append(lat)
    torch.cuda.synchronize()
    spec = LatentSpec(shape=shape, dtype=torch.float16, device=torch.device(DEV))
    for model in (eager, graphed):
        stage = PipelineStage(model, PipelineConfig(total_steps=steps, world_size=1, rank=0, timesteps=list(range(steps)),
                                                    latent_spec=spec, concurrent_samples=2))
        for trial in range(2 if model is graphed else 1):
            got = stage.run_many(n_samples, input_supplier=lambda i: xs[i],
                                 conditioning_supplier=lambda i, m=model: m.prepare_conditioning(embs[i], imgs[i],
                                                                                                 **settings(i)))
            torch.cuda.synchronize()
            for i in range(n_samples):
                assert torch.equal(got[i], want[i]), f"{'graphs' if model is graphed else 'eager'} trial {trial} sample {i}"
    assert len({k[0] for k in graphed._graphs}) == 2 and len(graphed._graphs) == 2 * steps
