"""Generate mode: a picture file in, the frames of a video out.

Counterpart of the ``main()`` of the reference's demo (``/root/reference/scripts/generate_video_demo.py:225-466``; same
flags where it has them, ``--output`` names the file instead of a directory of time-stamped names).  ``--model-id`` must be
a LOCAL checkpoint directory in the hub layout; ``--random-init`` runs the exact architecture with synthetic weights
(``--tiny``: the narrow test configuration).  Runs on one GPU as it is, or under torchrun as a step pipeline:

    python -m vdpp_amd.modes.generate --random-init --input-image in.png --output out.gif

``--window-frames W --window-stride S`` makes a video longer than the model's native frame count: ``--num-frames`` is then the
total, the conditioning is prepared for W frames, and every step denoises the long latent as overlapping windows of W frames
fused in the sampler update (``StableVideoUNet(window_stride=)``); decode and every output format
receive all ``--num-frames`` frames:

    python -m vdpp_amd.modes.generate --random-init --input-image in.png --num-frames 28 --window-frames 14 \
        --window-stride 7 --output out.gif

``--tile-height TH --tile-width TW --tile-stride-y SY --tile-stride-x SX`` (pixels, multiples of 8) make frames larger than the
model's native size: ``--height`` / ``--width`` are then the total, every step denoises the large latent as overlapping tiles of
TH x TW fused in the sampler update (``StableVideoUNet(tile_size=, tile_stride=)``), each tile conditioned
on its own crop of the image latents; decode, ``--interpolate`` and every output format receive the one large latent:

    python -m vdpp_amd.modes.generate --random-init --input-image in.png --height 576 --width 2048 --tile-height 576 \
        --tile-width 1024 --tile-stride-y 576 --tile-stride-x 512 --output out.gif

Every rank builds the conditioning from the file itself -- the image kernels, CLIP and the VAE encoder are deterministic
and the augmentation noise comes from a seeded CPU generator, so nothing is broadcast (the reference encodes on every rank
as well, ref ``:250-300``).  The steps go through ``run_pipeline_latents`` as in ``production.py``; the rank that ends up
with the finished latents decodes them to 8-bit frames (``decode_latents_uint8``) and writes them (``image_io.save_frames``:
``.avi`` -- Motion-JPEG, the video file; its frames, like those of a ``%03d.jpg`` pattern, are compressed on the GPU at
``--jpeg-quality`` and only the compressed bytes come to the host -- ``.gif``, the animated GIF of the demo: quantised to a
palette per frame and LZW-coded on the GPU as well (``image_io.GifEncoder``), at ``--fps`` -- ``.npy``, a ``%03d.png`` pattern
or a directory of PNGs, and ``.apng``, one lossless animated PNG at ``--fps``: PNG rows are filtered and deflated on the GPU
too (``image_io.PngEncoder``) -- and ``.webp``, lossless WebP in full colour that a browser plays: one animated file at
``--fps``, or with a ``%03d.webp`` pattern one still per frame, transformed and entropy-coded on the GPU
(``image_io.WebpEncoder``)).  The frames go to ``save_frames`` as the device tensor they are.  ``--interpolate 2`` / ``4`` puts
motion-compensated frames between the generated ones first, on the GPU (``image_io.FrameInterpolator``; ``--interp-range``,
``--interp-penalty``), and writes at ``--fps`` times that factor, so the video lasts as long.

``--input-decode device`` decodes a baseline JPEG picture on the GPU from its compressed bytes (``image_io.load_image_device``:
only plan and entropy-coded segment are uploaded; files outside the device decoder's scope still go through Pillow); the
default, ``host``, is Pillow's decode and the upload of the pixels, as before.
"""

from __future__ import annotations

import argparse
import logging
import os
import tempfile

import torch

from ..distributed import finalize_distributed, init_distributed, resolve_backend
from ..pipeline import LatentSpec, run_pipeline_latents

LOGGER = logging.getLogger(__name__)


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Generate video frames from an image (SVD step pipeline)")
    p.add_argument("--input-image", type=str, required=True, help="picture file (anything Pillow decodes)")
    p.add_argument("--output", type=str, required=True, help=".avi (Motion-JPEG video), .gif, .apng (lossless animated PNG), .webp (lossless animated WebP), .npy, a %%03d.jpg, %%03d.png or %%03d.webp pattern, or a directory for PNG frames")
    p.add_argument("--input-decode", type=str, default="host", choices=["host", "device"],
                   help="host: Pillow decodes the picture; device: a baseline JPEG is decoded on the GPU from its compressed bytes (other files still go through Pillow)")
    p.add_argument("--height", type=int, default=576)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--num-frames", type=int, default=14)
    p.add_argument("--window-frames", type=int, default=None,
                   help="long videos: the model's native frame count W; --num-frames is then the total, denoised as "
                        "overlapping windows of W frames (needs --window-stride)")
    p.add_argument("--window-stride", type=int, default=None,
                   help="frames between the starts of consecutive windows, from 1 to W; --num-frames must be W plus a whole "
                        "number of strides")
    p.add_argument("--window-weights", type=str, default="triangle", choices=["triangle", "uniform"],
                   help="how the windows covering a frame are blended: weighted most at a window's centre, or equally")
    p.add_argument("--tile-height", type=int, default=None,
                   help="large frames: the model's native height in pixels; --height is then the total, denoised as "
                        "overlapping tiles (needs --tile-width, --tile-stride-y and --tile-stride-x; multiples of 8)")
    p.add_argument("--tile-width", type=int, default=None, help="the model's native width in pixels; --width is then the total")
    p.add_argument("--tile-stride-y", type=int, default=None,
                   help="pixels between the tops of consecutive tiles, from 8 to --tile-height; --height must be the tile "
                        "height plus a whole number of strides")
    p.add_argument("--tile-stride-x", type=int, default=None, help="the same along the width")
    p.add_argument("--tile-weights", type=str, default="triangle", choices=["triangle", "uniform"],
                   help="how the tiles covering a pixel are blended: weighted most at a tile's centre, or equally")
    p.add_argument("--total-steps", type=int, default=25)
    p.add_argument("--sampler", type=str, default="euler", choices=["euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde"],
                   help="euler: the reference's first-order update; dpmpp_2m: DPM-Solver++(2M), second order at one UNet "
                        "evaluation per step (its history travels in the latent; the steps run in index order); euler_a, "
                        "dpmpp_2m_sde: their stochastic forms, fresh noise at every step from the sample's seed")
    p.add_argument("--eta", type=float, default=1.0, help="stochastic samplers: how much noise a step adds (0: none)")
    p.add_argument("--s-noise", type=float, default=1.0, help="stochastic samplers: scale of the added noise")
    p.add_argument("--noise", type=str, default="torch", choices=["torch", "device"],
                   help="the initial latent: torch.randn under the sample's seed, or the counter-based device generator, "
                        "whose values depend on the sample's seed and shape alone")
    p.add_argument("--fps", type=int, default=7)
    p.add_argument("--jpeg-quality", type=int, default=90, help="quality (1-100) of .avi / .jpg frames")
    p.add_argument("--interpolate", type=int, default=1, choices=[1, 2, 4],
                   help="frame-rate factor: put 1 or 3 motion-compensated frames between the generated ones on the GPU and "
                        "write at --fps times this, so the video lasts as long (1: off)")
    p.add_argument("--interp-range", type=int, default=16, help="--interpolate: motion search range in pixels (1-24)")
    p.add_argument("--interp-penalty", type=int, default=4, help="--interpolate: cost per pixel of vector length (0-255)")
    p.add_argument("--motion-bucket-id", type=int, default=127)
    p.add_argument("--noise-aug-strength", type=float, default=0.02)
    p.add_argument("--guidance-scale", type=float, default=3.0, help="CFG guidance scale (1.0 disables CFG)")
    p.add_argument("--num-samples", type=int, default=1, help="videos to generate (seed, seed+1, ...)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--model-id", type=str, default=None, help="LOCAL checkpoint directory in the hub layout")
    p.add_argument("--random-init", action="store_true")
    p.add_argument("--tiny", action="store_true", help="with --random-init: the narrow test configuration")
    p.add_argument("--decode-chunk-size", type=int, default=14)
    p.add_argument("--balanced", action="store_true")
    p.add_argument("--backend", type=str, default="auto", choices=["auto", "gloo", "nccl"])
    p.add_argument("--init-method", type=str, default=None)
    p.add_argument("--log-level", type=str, default="INFO")
    args = p.parse_args(argv)
    if args.random_init == bool(args.model_id):
        p.error("give exactly one of --model-id <local dir> and --random-init")
    if args.tiny and not args.random_init:
        p.error("--tiny needs --random-init")
    if args.eta < 0 or args.s_noise < 0:
        p.error("--eta and --s-noise must not be negative")
    if (args.noise == "device" or args.sampler in ("euler_a", "dpmpp_2m_sde")) \
            and not (0 <= args.seed and args.seed + args.num_samples <= 2 ** 63):
        p.error("--seed .. --seed + --num-samples - 1 must lie in [0, 2^63) for the device generator")
    if not 1 <= args.jpeg_quality <= 100:
        p.error("--jpeg-quality must be from 1 to 100")
    if not 1 <= args.interp_range <= 24 or not 0 <= args.interp_penalty <= 255:
        p.error("--interp-range must be from 1 to 24 and --interp-penalty from 0 to 255")
    if args.height % 8 or args.width % 8:
        p.error("--height and --width must be multiples of 8")
    if (args.window_frames is None) != (args.window_stride is None):
        p.error("--window-frames and --window-stride go together")
    if args.window_frames is not None:
        from ..models import window_plan

        w, st = args.window_frames, args.window_stride
        if w < 1 or not 1 <= st <= w:
            p.error(f"--window-stride {st} must be from 1 to --window-frames {w}")
        if args.num_frames < w:
            p.error(f"--num-frames {args.num_frames} is less than --window-frames {w}: the total must be at least one window; "
                    f"the nearest legal totals are {w} and {w + st}")
        if (args.num_frames - w) % st:
            lo, hi = window_plan.legal_totals(args.num_frames, w, st)
            p.error(f"--num-frames {args.num_frames} is not --window-frames {w} plus a whole number of strides of {st}: "
                    f"the nearest legal totals are {lo} and {hi}")
    tiles = (args.tile_height, args.tile_width, args.tile_stride_y, args.tile_stride_x)
    if any(v is not None for v in tiles) and any(v is None for v in tiles):
        p.error("--tile-height, --tile-width, --tile-stride-y and --tile-stride-x go together")
    if args.tile_height is not None:
        from ..models import tile_plan

        if any(v % 8 for v in tiles):
            p.error("--tile-height, --tile-width, --tile-stride-y and --tile-stride-x must be multiples of 8")
        for axis, flag, total, t, st in (("y", "height", args.height, args.tile_height, args.tile_stride_y),
                                         ("x", "width", args.width, args.tile_width, args.tile_stride_x)):
            if t < 8 or not 8 <= st <= t:
                p.error(f"--tile-stride-{axis} {st} must be from 8 to --tile-{flag} {t}")
            if total < t:
                p.error(f"--{flag} {total} is less than --tile-{flag} {t}: the total must be at least one tile; "
                        f"the nearest legal totals are {t} and {t + st}")
            if (total - t) % st:
                lo, hi = tile_plan.legal_totals(total // 8, t // 8, st // 8)
                p.error(f"--{flag} {total} is not --tile-{flag} {t} plus a whole number of strides of {st}: "
                        f"the nearest legal totals are {8 * lo} and {8 * hi}")
    return args


def tile_arguments(args) -> dict:
    """``tile_size`` / ``tile_stride`` / ``tile_weights`` of ``StableVideoUNet`` in latent cells; empty without tiles."""
    if args.tile_height is None:
        return {}
    return dict(tile_size=(args.tile_height // 8, args.tile_width // 8),
                tile_stride=(args.tile_stride_y // 8, args.tile_stride_x // 8), tile_weights=args.tile_weights)


def sample_output_path(path: str, index: int, num_samples: int) -> str:
    """``path`` for a single video, else the sample index goes in front of the extension (``out_s1.gif``, ``frames_s1``)."""
    if num_samples == 1:
        return path
    root, ext = os.path.splitext(path)
    return f"{root}_s{index}{ext}"


def _clip_normalisation(model_dir):
    """``(image_mean, image_std)`` of ``<model_dir>/feature_extractor/preprocessor_config.json`` (ref ``:256-258``), or
    ``(None, None)`` -- the front end's OpenAI CLIP constants -- without that file."""
    import json

    path = os.path.join(model_dir or "", "feature_extractor", "preprocessor_config.json")
    if not os.path.exists(path):
        return None, None
    with open(path) as fh:
        cfg = json.load(fh)
    return cfg.get("image_mean"), cfg.get("image_std")


def _build_engines(args, timesteps, device):
    """``(model, clip, vae_encoder, make_decoder)``: the decoder is built only on the rank that decodes."""
    from ..models.clip_hip import CLIPVisionHIP, CLIPVisionSpec
    from ..models.clip_hip import random_state_dict as clip_random_state_dict
    from ..models.svd_unet import StableVideoUNet
    from ..models.unet_spec import UNetConfig
    from ..models.vae_hip import (ImageEncoderHIP, TemporalDecoderHIP, VAEDecoderConfig, random_encoder_state_dict,
                                  random_state_dict)

    if args.random_init:
        ucfg = UNetConfig.tiny(64) if args.tiny else UNetConfig.svd()
        spec = CLIPVisionSpec.tiny(ucfg.cross_attention_dim) if args.tiny else CLIPVisionSpec.svd()
        vcfg = VAEDecoderConfig.tiny(64) if args.tiny else VAEDecoderConfig.svd()
        model = StableVideoUNet.from_random_init(timesteps, config=ucfg, seed=args.seed, device=device, sampler=args.sampler,
                                                 window_stride=args.window_stride, window_weights=args.window_weights,
                                                 eta=args.eta, s_noise=args.s_noise, **tile_arguments(args))
        clip = CLIPVisionHIP(spec, clip_random_state_dict(spec, seed=args.seed + 1, device=device), device)
        enc = ImageEncoderHIP(vcfg, random_encoder_state_dict(vcfg, seed=args.seed + 2, device=device), device)
        return model, clip, enc, lambda: TemporalDecoderHIP(vcfg, random_state_dict(vcfg, seed=args.seed + 3, device=device),
                                                            device)
    from ..models.edge_stages import load_edge_engines

    model = StableVideoUNet.from_pretrained(args.model_id, timesteps=timesteps, device=device, sampler=args.sampler,
                                            window_stride=args.window_stride, window_weights=args.window_weights,
                                            eta=args.eta, s_noise=args.s_noise, **tile_arguments(args))
    clip, enc, dec = load_edge_engines(args.model_id, device)
    return model, clip, enc, lambda: dec


def _step_order(sampler: str, total_steps: int) -> list:
    """The ``step`` values the pipeline hands to the model, in order.  Euler keeps the reference modes' descending list
    (``production.py:88``: the value is passed verbatim); a multistep solver needs the previous
    step's estimate and walks the sigma table in index order, and so do the stochastic samplers."""
    return list(range(total_steps)) if sampler != "euler" else list(range(total_steps - 1, -1, -1))


def main(argv=None) -> None:
    from ..models.edge_stages import encode_image_u8
    from ..models.image_io import ImageFrontEnd, load_image, load_image_device, save_frames
    from ..models.svd_unet import StableVideoUNet

    args = parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper()),
                        format="%(asctime)s %(levelname)s %(name)s: %(message)s")
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    device = torch.device(f"cuda:{local_rank}")
    torch.cuda.set_device(device)
    # before the process group: a missing file fails alone
    image = load_image_device(args.input_image, device) if args.input_decode == "device" else load_image(args.input_image)
    # one process started without torchrun: nothing is ever sent, the group only has to exist (Gloo, rendezvous in a file)
    alone = world == 1 and args.init_method is None and "MASTER_ADDR" not in os.environ
    backend = resolve_backend(None if args.backend == "auto" else args.backend, simulator=alone and args.backend == "auto")
    rendezvous = tempfile.TemporaryDirectory() if alone else None
    init_method = f"file://{rendezvous.name}/rendezvous" if alone else args.init_method
    init_distributed(backend=backend, rank=rank, world_size=world, init_method=init_method)
    try:
        with torch.no_grad():
            timesteps = StableVideoUNet._default_timestep_schedule(args.total_steps)
            model, clip, enc, make_decoder = _build_engines(args, timesteps, device)
            mean, std = _clip_normalisation(args.model_id)
            front = ImageFrontEnd(device, args.height, args.width, clip_size=clip.spec.image_size, clip_mean=mean, clip_std=std)
            noise = torch.randn((1, 3, args.height, args.width), generator=torch.Generator().manual_seed(args.seed))
            # with windows the model is conditioned for one window; the latent, the decode and the file hold the total
            cond_frames = args.window_frames or args.num_frames
            emb, image_latents = encode_image_u8(image, front, clip, enc, cond_frames, noise=noise,
                                                 noise_aug_strength=args.noise_aug_strength)
            del clip, enc, front
            model.set_conditioning(emb, image_latents, fps=args.fps, motion_bucket_id=args.motion_bucket_id,
                                   noise_aug_strength=args.noise_aug_strength, guidance_scale=args.guidance_scale,
                                   num_frames=cond_frames)
            if args.window_frames is not None:
                from ..models import window_plan

                shape = torch.Size(window_plan.noise_shape(1, args.num_frames, args.height, args.width, args.window_frames,
                                                           args.window_stride))
            elif args.tile_height is not None:
                from ..models import tile_plan

                shape = torch.Size(tile_plan.noise_shape(1, args.num_frames, args.height, args.width, args.tile_height,
                                                         args.tile_width, args.tile_stride_y, args.tile_stride_x))
            else:
                shape = torch.Size((1, 4, args.num_frames, args.height // 8, args.width // 8))
            # what a stage boundary carries: the sample, and with dpmpp_2m the solver's history behind it (8 channels)
            carried = torch.Size((1, model.state_channels) + tuple(shape[2:]))
            spec = LatentSpec(shape=carried, dtype=torch.float16, device=device)

            def supplier(i: int) -> torch.Tensor:
                if args.noise == "device":
                    return model.init_state(model.initial_noise(args.seed + i, *shape[2:]))
                torch.manual_seed(args.seed + i)
                return model.init_state(torch.randn(shape, device=device, dtype=torch.float16) * model.init_noise_sigma)

            # a stochastic sampler draws sample i's step noise from seed + i: the model's one conditioning with that seed,
            # handed to every step of the sample on whichever rank runs it
            conditioning, seeded = None, {}
            if model.stochastic:
                def conditioning(i: int):
                    if i not in seeded:
                        seeded[i] = model.conditioning.with_noise_seed(args.seed + i)
                    return seeded[i]

            outs = run_pipeline_latents(model, total_steps=args.total_steps,
                                        timesteps=_step_order(args.sampler, args.total_steps), world_size=world,
                                        rank=rank, latent_spec=spec, num_samples=args.num_samples,
                                        input_supplier=supplier if rank == 0 else None, balanced=args.balanced,
                                        conditioning_supplier=conditioning)
            if outs:
                decoder = make_decoder()
                for i, latents in enumerate(outs):
                    frames = decoder.decode_latents_uint8(model.sample_of(latents).contiguous(), args.num_frames,
                                                          decode_chunk_size=args.decode_chunk_size)
                    # the device tensor goes in as it is: .avi / .jpg frames are compressed where they are
                    files = save_frames(frames[0], sample_output_path(args.output, i, args.num_samples), args.fps,
                                        quality=args.jpeg_quality, interpolate=args.interpolate, interp_range=args.interp_range,
                                        interp_penalty=args.interp_penalty)
                    LOGGER.info("sample %d (seed %d): %d frames of %dx%d -> %s", i, args.seed + i, frames.shape[1],
                                frames.shape[3], frames.shape[2], files[0] if len(files) == 1 else os.path.dirname(files[0]))
                    if args.interpolate > 1:
                        LOGGER.info("sample %d: interpolated %d frames at %d fps to %d at %d fps (range %d, penalty %d)", i,
                                    frames.shape[1], args.fps, (frames.shape[1] - 1) * args.interpolate + 1,
                                    args.fps * args.interpolate, args.interp_range, args.interp_penalty)
    finally:
        finalize_distributed()
        if rendezvous is not None:
            rendezvous.cleanup()


if __name__ == "__main__":
    main()
