"""Image front end, 8-bit frame output and the generate mode on the GPU.

The resize kernels are held against Pillow itself, the CLIP preprocessing against transformers' ``CLIPImageProcessor``
and the cover-resize / crop against the reference's ``load_and_preprocess_image``
(/root/reference/scripts/generate_video_demo.py:71-89), all through tests/golden/image_io.npz
(tests/golden/make_image_golden.py).  Cap for every uint8 comparison with Pillow: no value more than ONE level off, and
at most 2 % of a case's values off at all -- Pillow's weights are 22-bit fixed point, the kernel's fp32; the minter
measured an fp64 statement of the same algorithm at <= 0.22 % on these cases and refuses a case above 1.5 %.
The frame conversions have exact references and are compared byte for byte."""

import os

import numpy as np
import pytest
import torch

from tests.golden import make_image_golden as mint

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEVELS, MAX_SHARE = 1, 0.02
FP16_STEP = 2.0 ** -9          # one fp16 spacing at the largest magnitude the normalised tensors reach (2.15 < 4)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "image_io.npz"))


def _ops():
    from vdpp_amd.hip import ops
    return ops


def _under_cap(got, want, what):
    worst, share = mint.compare_levels(got, want)
    print(f"{what}: largest difference {worst} level(s), {share:.3%} of the values differ")
    assert worst <= MAX_LEVELS, f"{what}: {worst} levels off Pillow"
    assert share <= MAX_SHARE, f"{what}: {share:.2%} of the values differ from Pillow"


def _view(h, w, pitch, offset, fill):
    """(h, w, 3) uint8 view with a padded row pitch and a byte offset into a larger buffer filled with `fill`."""
    buf = torch.full((offset + h * pitch + 16,), fill, dtype=torch.uint8, device=DEV)
    return buf, torch.as_strided(buf, (h, w, 3), (pitch, 3, 1), offset)


@pytest.mark.parametrize("case", range(len(mint.RAW_CASES)))
def test_resample_matches_pillow(golden, case):
    ops = _ops()
    (sh, sw), (dh, dw), filt = mint.RAW_CASES[case]
    f = ops.FILTER_LANCZOS3 if filt == "L" else ops.FILTER_BICUBIC
    tmp = torch.empty(ops.image_resample_tmp_bytes(sh, dw), dtype=torch.uint8, device=DEV)
    for kind in mint.KINDS:
        src = mint.source_image(kind, sh, sw, mint.case_seed(0, case, kind))
        want = golden[f"raw{case}_{kind}"]
        dst = torch.empty((dh, dw, 3), dtype=torch.uint8, device=DEV)
        ops.image_resample_u8(torch.from_numpy(src).to(DEV), dst, tmp, filter=f)
        _under_cap(dst.cpu().numpy(), want, f"{sh}x{sw} -> {dh}x{dw} {filt} {kind}")
    # the same through views into larger buffers: odd base offsets, row pitches that are no multiple of anything
    _, sview = _view(sh, sw, 3 * sw + 7, 5, 0)
    sview.copy_(torch.from_numpy(src).to(DEV))
    dbuf, dview = _view(dh, dw, 3 * dw + 5, 3, 0xAB)
    ops.image_resample_u8(sview, dview, tmp, filter=f)
    assert torch.equal(dview, dst), "a padded pitch / odd offset changes the result"
    mask = torch.ones_like(dbuf, dtype=torch.bool)
    torch.as_strided(mask, (dh, dw, 3), (3 * dw + 5, 3, 1), 3).fill_(False)
    assert bool((dbuf[mask] == 0xAB).all()), "bytes outside the destination view were written"


def test_resample_wrapper_refuses_bad_arguments():
    ops = _ops()
    src = torch.zeros((4, 10, 3), dtype=torch.uint8, device=DEV)
    dst = torch.zeros((2, 5, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ops.HipKernelError, match="tmp"):
        ops.image_resample_u8(src, dst, torch.empty(4 * 5 * 3 - 1, dtype=torch.uint8, device=DEV), filter=ops.FILTER_LANCZOS3)
    with pytest.raises(ops.HipKernelError, match="filter"):
        ops.image_resample_u8(src, dst, torch.empty(60, dtype=torch.uint8, device=DEV), filter=7)
    with pytest.raises(ValueError):
        ops.image_resample_u8(src.permute(1, 0, 2), dst, torch.empty(60, dtype=torch.uint8, device=DEV), filter=0)


@pytest.mark.parametrize("which", ["vae", "clip"])
def test_image_to_tensor_every_level(golden, which):
    """16x48 pixels hold all 256 levels in every channel (three times over, in a different order per channel); against
    the fp32 formula rounded to fp16."""
    ops = _ops()
    mean, std = ((0.5,) * 3, (0.5,) * 3) if which == "vae" else (golden["clip_mean"].tolist(), golden["clip_std"].tolist())
    i = np.arange(16 * 48)
    img = np.stack([i % 256, (i * 7 + 3) % 256, (255 - i * 5) % 256], axis=-1).astype(np.uint8).reshape(16, 48, 3)
    assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    m, s = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1), torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    want = ((torch.from_numpy(img).permute(2, 0, 1).float() / 255.0 - m) / s).half().float()
    assert float(want.abs().max()) < 4.0
    _, view = _view(16, 48, 3 * 48 + 11, 1, 0)
    view.copy_(torch.from_numpy(img).to(DEV))
    for src in (torch.from_numpy(img).to(DEV), view):
        out = torch.full((3, 16, 48), 9.0, dtype=torch.float16, device=DEV)
        ops.image_to_tensor(src, out, mean=mean, std=std)
        err = float((out.float().cpu() - want).abs().max())
        print(f"image_to_tensor {which}: max abs error {err:.3e}")
        assert err <= FP16_STEP


def test_front_end_matches_the_reference_chain(golden):
    from vdpp_amd.models.image_io import ImageFrontEnd, clip_geometry, cover_geometry
    fe = ImageFrontEnd(DEV, mint.TARGET_H, mint.TARGET_W, clip_size=mint.CLIP_SIZE)
    assert np.allclose(fe.clip_mean, golden["clip_mean"]) and np.allclose(fe.clip_std, golden["clip_std"])
    std = torch.tensor(golden["clip_std"], dtype=torch.float32).view(1, 3, 1, 1)
    for i, ((sh, sw), kind) in enumerate(mint.CHAIN_CASES):
        src = mint.source_image(kind, sh, sw, mint.case_seed(1, i, kind))
        geo = golden[f"chain{i}_geometry"].tolist()
        assert list(cover_geometry(sh, sw, mint.TARGET_H, mint.TARGET_W)) == geo[:4]
        assert list(clip_geometry(mint.TARGET_H, mint.TARGET_W, mint.CLIP_SIZE)) == geo[4:]
        # an ndarray, a tensor, and a non-contiguous view of the same picture give the same three results
        pv, it, crop = fe(src)
        wide = np.zeros((sh, sw + 3, 4), np.uint8)
        wide[:, :sw, :3] = src
        pv2, it2, crop2 = fe(torch.from_numpy(wide)[:, :sw, :3])
        assert torch.equal(pv, pv2) and torch.equal(it, it2) and torch.equal(crop, crop2)
        assert pv.shape == (1, 3, mint.CLIP_SIZE, mint.CLIP_SIZE) and pv.dtype == torch.float16
        assert it.shape == (1, 3, mint.TARGET_H, mint.TARGET_W) and it.dtype == torch.float16
        assert crop.shape == (mint.TARGET_H, mint.TARGET_W, 3) and crop.dtype == torch.uint8 and crop.is_contiguous()
        want_crop = golden[f"chain{i}_cropped"]
        if (sh, sw) == (mint.TARGET_H, mint.TARGET_W):
            assert np.array_equal(crop.cpu().numpy(), src) and np.array_equal(want_crop, src)
        _under_cap(crop.cpu().numpy(), want_crop, f"chain {sh}x{sw} {kind}: cropped image")
        half = torch.full((1, 3, 1, 1), 0.5)
        for name, got, want, level in (("image_tensor", it, golden[f"chain{i}_image_tensor"], 1.0 / (255.0 * half)),
                                       ("pixel_values", pv, golden[f"chain{i}_pixel_values"], 1.0 / (255.0 * std))):
            d = (got.float().cpu() - torch.from_numpy(want)[None]).abs()
            share = float((d > FP16_STEP).float().mean())
            print(f"chain {sh}x{sw} {kind}: {name} max error {float((d / level).max()):.3f} levels, {share:.3%} beyond 2^-9")
            assert bool((d <= level + FP16_STEP).all()), f"{name}: more than one level off the reference"
            assert share <= MAX_SHARE, f"{name}: {share:.2%} of the entries are beyond fp16 rounding"


def _frame_values():
    """Every exact level boundary 2k/255 - 1 with its two fp32 neighbours, +-inf, and uniform values over [-1.5, 1.5]."""
    k = np.arange(256, dtype=np.float64)
    edge = (2.0 * k / 255.0 - 1.0).astype(np.float32)
    special = np.concatenate([edge, np.nextafter(edge, np.float32(-9)), np.nextafter(edge, np.float32(9)),
                              np.array([np.inf, -np.inf, 1.5, -1.5, 0.0, -0.0], np.float32)])
    n = 2 * 3 * 3 * 6 * 20
    rest = np.random.RandomState(5).uniform(-1.5, 1.5, n - len(special)).astype(np.float32)
    v = np.concatenate([special, rest])
    np.random.RandomState(6).shuffle(v)
    return torch.from_numpy(v).reshape(2, 3, 3, 6, 20)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_frames_to_uint8_is_the_reference_expression(dtype):
    from vdpp_amd.models.image_io import frames_to_uint8
    x = _frame_values().to(dtype)
    want = ((x.float() + 1) / 2 * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()
    got = frames_to_uint8(x.to(DEV))
    assert got.shape == (2, 3, 6, 20, 3) and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), want)
    # a plane size that is no multiple of four pixels takes the one-pixel path; a NaN is level 0 by definition
    y = x[:, :, :, :5, :3].contiguous()
    y[0, 1, 2, 3, 1] = float("nan")
    got = frames_to_uint8(y.to(DEV)).cpu()
    ref = torch.nan_to_num(y.float(), nan=-1.0)
    assert torch.equal(got, ((ref + 1) / 2 * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1))
    assert int(got[0, 2, 3, 1, 1]) == 0
    z = x.clone()
    z[1, 2, 0, 4, 7] = float("nan")
    assert int(frames_to_uint8(z.to(DEV))[1, 0, 4, 7, 2]) == 0


@pytest.fixture(scope="module")
def decoder():
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    vcfg = VAEDecoderConfig.tiny(64)
    return TemporalDecoderHIP(vcfg, random_state_dict(vcfg, seed=19), DEV)


@pytest.mark.parametrize("chunk", [2, 3, 14])
def test_decode_latents_uint8_equals_conversion_of_the_fp32_decode(decoder, chunk):
    """Chunks of 2 straddle the two 3-frame videos; byte for byte the conversion of decode_latents with the same chunks."""
    from vdpp_amd.models.edge_stages import decode_latents, decode_latents_uint8
    from vdpp_amd.models.image_io import frames_to_uint8
    lat = (torch.randn(2, 4, 3, 8, 16, generator=torch.Generator().manual_seed(3)) * 0.8).half().to(DEV)
    frames = decode_latents(lat, decoder, 3, decode_chunk_size=chunk)
    want = frames_to_uint8(frames)
    got = decode_latents_uint8(lat, decoder, 3, decode_chunk_size=chunk)
    assert got.shape == (2, 3, 64, 128, 3) and got.dtype == torch.uint8
    assert torch.equal(got, want)
    assert len(torch.unique(got)) > 2, "a decode that only saturates shows nothing"
    cpu = ((frames.cpu() + 1) / 2 * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1)
    assert torch.equal(got.cpu(), cpu)


def test_frame_emitter_uint8_output(decoder):
    from vdpp_amd.models.edge_stages import FrameEmitter
    from vdpp_amd.models.image_io import frames_to_uint8
    from vdpp_amd.models.svd_unet import StableVideoUNet
    from vdpp_amd.models.unet_hip import SVDUNetHIP
    from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict
    from vdpp_amd.pipeline import LatentSpec, PipelineConfig, PipelineStage
    dev = torch.device(DEV)
    ucfg = UNetConfig.tiny(64)
    model = StableVideoUNet(unet=SVDUNetHIP(ucfg, random_state_dict(ucfg, seed=0, dtype=torch.float16), dev),
                            timesteps=StableVideoUNet._default_timestep_schedule(2))
    torch.manual_seed(42)
    model.set_dummy_conditioning(1, 3, 8, 16, dev)
    spec = LatentSpec(shape=torch.Size((1, 4, 3, 8, 16)), dtype=torch.float16, device=dev)

    def supplier(i):
        g = torch.Generator().manual_seed(1000 + i)
        return (torch.randn(spec.shape, generator=g) * model.init_noise_sigma).half().to(dev)

    def run(samples, **kw):
        stage = PipelineStage(model, PipelineConfig(total_steps=2, timesteps=[0, 1], world_size=1, rank=0, latent_spec=spec))
        emitter = FrameEmitter(decoder, stage, 3, **kw)
        with torch.no_grad():
            out = stage.run_many(samples, input_supplier=supplier)
            stage.drain()
            return emitter, out, emitter.finish(samples)

    emitter, out, frames = run(2, output="uint8")
    assert emitter.output == "uint8" and sorted(frames) == [0, 1]
    with torch.no_grad():
        for i in range(2):
            want = frames_to_uint8(decoder.decode_latents(out[i].contiguous(), 3))
            assert frames[i].dtype == torch.uint8 and frames[i].shape == (1, 3, 64, 128, 3)
            assert torch.equal(frames[i], want)
    emitter, out, frames = run(1)
    assert emitter.output == "float32"
    with torch.no_grad():
        assert frames[0].dtype == torch.float32 and torch.equal(frames[0], decoder.decode_latents(out[0].contiguous(), 3))
    with pytest.raises(ValueError):
        FrameEmitter(decoder, emitter.stage, 3, output="int8")


def test_encode_image_u8_is_front_end_plus_encode_image(golden, golden_dir):
    from tests.golden.make_clip_golden import CFG
    from vdpp_amd.models.clip_hip import CLIPVisionHIP, CLIPVisionSpec
    from vdpp_amd.models.edge_stages import encode_image, encode_image_u8
    from vdpp_amd.models.image_io import ImageFrontEnd
    from vdpp_amd.models.vae_hip import ImageEncoderHIP, VAEDecoderConfig, random_encoder_state_dict
    z = np.load(os.path.join(golden_dir, "clip_tiny.npz"))
    spec = CLIPVisionSpec(CFG["hidden_size"], CFG["intermediate_size"], CFG["num_hidden_layers"], CFG["num_attention_heads"],
                          CFG["image_size"], CFG["patch_size"], CFG["projection_dim"], CFG["layer_norm_eps"], CFG["hidden_act"])
    clip = CLIPVisionHIP(spec, {k[2:]: torch.from_numpy(z[k]).half() for k in z.files if k.startswith("w:")}, DEV)
    vcfg = VAEDecoderConfig.tiny(64)
    enc = ImageEncoderHIP(vcfg, random_encoder_state_dict(vcfg, seed=4), DEV)
    fe = ImageFrontEnd(DEV, mint.TARGET_H, mint.TARGET_W, clip_size=spec.image_size)
    (sh, sw), kind = mint.CHAIN_CASES[1]
    img = mint.source_image(kind, sh, sw, mint.case_seed(1, 1, kind))
    noise = torch.randn(1, 3, mint.TARGET_H, mint.TARGET_W, generator=torch.Generator().manual_seed(8))
    for kw in (dict(), dict(noise=noise, noise_aug_strength=0.02)):
        emb, lat = encode_image_u8(img, fe, clip, enc, 3, **kw)
        pv, it, _ = fe(img)
        emb2, lat2 = encode_image(pv, it, clip, enc, 3, **kw)
        assert emb.shape == (1, 1, CFG["projection_dim"]) and lat.shape == (1, 4, 3, mint.TARGET_H // 8, mint.TARGET_W // 8)
        assert torch.isfinite(emb).all() and torch.isfinite(lat).all()
        assert torch.equal(emb, emb2) and torch.equal(lat, lat2)


def test_generate_mode_writes_frames(monkeypatch, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.modes import generate
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    (sh, sw), kind = mint.CHAIN_CASES[0]
    src = tmp_path / "in.png"
    Image.fromarray(mint.source_image(kind, sh, sw, mint.case_seed(1, 0, kind))).save(src)

    def run(out, tag):
        generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_{tag}", "--log-level", "WARNING",
                       "--random-init", "--tiny", "--input-image", str(src), "--height", "64", "--width", "128",
                       "--num-frames", "3", "--total-steps", "2", "--output", str(out)])
        assert not torch.distributed.is_initialized()

    run(tmp_path / "x.gif", "gif")
    with Image.open(tmp_path / "x.gif") as im:
        assert im.n_frames == 3 and im.size == (128, 64)
    run(tmp_path / "x.npy", "a")
    a = np.load(tmp_path / "x.npy")
    assert a.shape == (3, 64, 128, 3) and a.dtype == np.uint8
    assert int(a.max()) > int(a.min()), "constant frames"
    run(tmp_path / "y.npy", "b")
    assert np.array_equal(a, np.load(tmp_path / "y.npy")), "the same seed gave other frames"
