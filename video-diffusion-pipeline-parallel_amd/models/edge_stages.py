"""What the first and the last pipeline stage do around the denoising steps, as the reference's demo arranges it
(``/root/reference/scripts/generate_video_demo.py``): ``encode_image`` on rank 0 (``:92-151``) and ``decode_latents`` on
the last rank (``:154-195``), on the HIP engines of ``clip_hip.py`` / ``vae_hip.py``.

Same argument meaning and return values as the script's functions, minus what is host-side image handling there: the
``CLIPImageProcessor`` output (``pixel_values``) and the normalised image tensor are arguments instead of a PIL image.
``encode_image_u8`` takes the picture itself (uint8 pixels) and makes those two tensors on the device
(``image_io.ImageFrontEnd``); ``decode_latents_uint8`` / ``FrameEmitter(output="uint8")`` end in the 8-bit frames the
script's ``save_video`` writes, ``FrameEmitter(output="jpeg")`` in those frames compressed (``image_io.JpegEncoder``).
"""

from __future__ import annotations

import torch

from .clip_hip import CLIPVisionHIP
from .vae_hip import ImageEncoderHIP, TemporalDecoderHIP


def _read_local_checkpoint(model_dir: str, subfolder: str) -> tuple[dict, dict]:
    """``(state_dict, config)`` of ``<model_dir>/<subfolder>`` in the hub layout (``*.safetensors`` -- the ``.fp16.`` variant
    when both are shipped -- and ``config.json``).  Local directories only: there is no network to fetch a model name."""
    import json
    import os

    sub = os.path.join(model_dir, subfolder)
    if not os.path.isdir(sub):
        raise ValueError(f"'{model_dir}' holds no '{subfolder}' directory: pass a LOCAL checkpoint directory in the hub "
                         f"layout (a model name cannot be fetched: no network access)")
    from safetensors.torch import load_file

    files = sorted(n for n in os.listdir(sub) if n.endswith(".safetensors"))
    fp16_files = [n for n in files if ".fp16." in n]
    sd = {}
    for name in (fp16_files or files):
        sd.update(load_file(os.path.join(sub, name)))
    if not sd:
        raise ValueError(f"no *.safetensors weights under '{sub}'")
    cfg = {}
    cfg_path = os.path.join(sub, "config.json")
    if os.path.exists(cfg_path):
        with open(cfg_path) as fh:
            cfg = json.load(fh)
    return sd, cfg


def load_edge_engines(model_dir: str, device="cuda"):
    """``(clip, vae_encoder, vae_decoder)`` from a local Stable Video Diffusion checkpoint directory, as the reference's
    demo loads them by id (``CLIPVisionModelWithProjection.from_pretrained(.., subfolder="image_encoder")``,
    ``AutoencoderKLTemporalDecoder.from_pretrained(.., subfolder="vae")``: ref ``scripts/generate_video_demo.py:248-262``)."""
    from .clip_hip import CLIPVisionSpec
    from .vae_hip import VAEDecoderConfig

    csd, ccfg = _read_local_checkpoint(model_dir, "image_encoder")
    d = CLIPVisionSpec()
    spec = CLIPVisionSpec(ccfg.get("hidden_size", d.hidden_size), ccfg.get("intermediate_size", d.intermediate_size),
                          ccfg.get("num_hidden_layers", d.num_hidden_layers), ccfg.get("num_attention_heads", d.num_attention_heads),
                          ccfg.get("image_size", d.image_size), ccfg.get("patch_size", d.patch_size),
                          ccfg.get("projection_dim", d.projection_dim), ccfg.get("layer_norm_eps", d.layer_norm_eps),
                          ccfg.get("hidden_act", d.hidden_act))
    clip = CLIPVisionHIP(spec, csd, device)
    vsd, vcfg = _read_local_checkpoint(model_dir, "vae")
    v = VAEDecoderConfig()
    cfg = VAEDecoderConfig(latent_channels=vcfg.get("latent_channels", v.latent_channels),
                           out_channels=vcfg.get("out_channels", v.out_channels),
                           block_out_channels=tuple(vcfg.get("block_out_channels", v.block_out_channels)),
                           layers_per_block=vcfg.get("layers_per_block", v.layers_per_block),
                           scaling_factor=vcfg.get("scaling_factor", v.scaling_factor))
    enc = ImageEncoderHIP(cfg, {k: t for k, t in vsd.items() if k.startswith(("encoder.", "quant_conv."))}, device)
    dec = TemporalDecoderHIP(cfg, {k[len("decoder."):]: t for k, t in vsd.items() if k.startswith("decoder.")}, device)
    return clip, enc, dec


def encode_image(pixel_values: torch.Tensor, image_tensor: torch.Tensor, image_encoder: CLIPVisionHIP,
                 vae_encoder: ImageEncoderHIP, num_frames: int, noise: torch.Tensor | None = None,
                 noise_aug_strength: float = 0.0) -> tuple[torch.Tensor, torch.Tensor]:
    """``(image_embeddings (B,1,1024), image_latents (B,4,F,H/8,W/8))`` as ``StableVideoUNet.set_conditioning`` takes
    them.  ``pixel_values``: ``feature_extractor(images=image).pixel_values`` (ref ``:108-109``); ``image_tensor``:
    ``Normalize([0.5],[0.5])(ToTensor(image))`` (ref ``:117-124``).  Noise augmentation in PIXEL space (ref ``:126-129``):
    the reference draws ``randn_like`` on its device; here the caller passes the ``noise`` tensor it wants added (device
    RNG streams differ between platforms), scaled by ``noise_aug_strength``.  The latents are the distribution's mode,
    NOT multiplied by the scaling factor (ref ``:139-142``)."""
    dev = image_encoder.device
    emb = image_encoder(pixel_values.to(dev, torch.float16).contiguous()).unsqueeze(1)
    img = image_tensor.to(dev, torch.float16)
    if noise is not None and noise_aug_strength > 0:
        img = torch.add(img, noise.to(dev, torch.float16), alpha=noise_aug_strength)    # input preparation, once per video
    latents = vae_encoder.encode_image_latents(img.contiguous(), num_frames)
    return emb, latents


def encode_image_u8(image_u8, front_end, image_encoder: CLIPVisionHIP, vae_encoder: ImageEncoderHIP, num_frames: int,
                    noise: torch.Tensor | None = None, noise_aug_strength: float = 0.0) -> tuple[torch.Tensor, torch.Tensor]:
    """``encode_image`` from the picture itself: ``image_u8`` (H, W, 3) uint8 of any size goes through ``front_end`` (an
    ``image_io.ImageFrontEnd``: the reference's cover-resize and crop, then the CLIP processor and ``ToTensor`` /
    ``Normalize`` on the cropped picture), the two tensors it returns through ``encode_image``.  ``noise``: as there,
    shaped like the image tensor (1, 3, height, width)."""
    pixel_values, image_tensor, _ = front_end(image_u8)
    return encode_image(pixel_values, image_tensor, image_encoder, vae_encoder, num_frames, noise=noise,
                        noise_aug_strength=noise_aug_strength)


def decode_latents(latents: torch.Tensor, vae: TemporalDecoderHIP, num_frames: int,
                   decode_chunk_size: int = 14) -> torch.Tensor:
    """(B, 4, F, H, W) latents -> (B, 3, F, 8H, 8W) fp32 frames (ref ``:154-195``)."""
    return vae.decode_latents(latents.to(vae.device, torch.float16).contiguous(), num_frames,
                              decode_chunk_size=decode_chunk_size)


def decode_latents_uint8(latents: torch.Tensor, vae: TemporalDecoderHIP, num_frames: int,
                         decode_chunk_size: int = 14) -> torch.Tensor:
    """(B, 4, F, H, W) latents -> (B, F, 8H, 8W, 3) uint8 frames: ``decode_latents`` and the conversion of ``save_video``
    (ref ``:205``) in one, without the fp32 video in between."""
    return vae.decode_latents_uint8(latents.to(vae.device, torch.float16).contiguous(), num_frames,
                                    decode_chunk_size=decode_chunk_size)


class FrameEmitter:
    """``decode_latents`` wired into the step pipeline, so that the node emits frames (ref
    ``scripts/generate_video_demo.py:418`` decodes every finished latent on the LAST rank, after the step loop).

    The temporal-VAE decode of one video costs about as much as a whole stage of an 8-GPU pipeline (three UNet steps).
    Every rank decodes what FINISHES on it, on a HIP stream of its own BESIDE its UNet steps, and never moves a finished
    latent:

      * ring schedule (``bench.py``'s default at N > 1): sample ``i`` finishes on rank ``(i mod N) - 1`` and is decoded
        right there, so per video each GPU carries 1/N of a decode;
      * chain of stages: everything finishes, and is decoded, on the last rank -- the reference's arrangement.

    Until round 4 the chain could also spread its decodes (sample ``i`` on rank ``i mod N``, the last rank forwarding the
    latent with ``isend(tag=7001)``).  That was removed: RCCL ignores tags and orders the un-batched P2P of a rank PAIR on
    one internal stream, so on the pair (N-2, N-1) the forwards shared a communicator with the stage hand-offs and, with
    two samples interleaved per rank, the two sides could issue the two directions in different orders (last rank:
    recv, recv, send -- rank N-2: recv, send, send) and wait for each other for ever.  Over Gloo (tags honoured, host
    threads) this cannot show.  Now no message exists whose order could cross: ``spread`` is accepted for older call
    sites and means "decode where the sample finishes", which balances the ring and leaves the chain on its last rank.

    Attach to a stage on EVERY rank (same arguments), run the pipeline, then ``finish(num_samples)``:

        emitter = FrameEmitter(decoder, stage, num_frames)            # every rank
        stage.run_many(K, input_supplier=...); stage.drain()
        frames = emitter.finish(K)                                    # {sample index: (B,3,F,8H,8W) fp32} decoded HERE

    ``output="uint8"`` keeps (B,F,8H,8W,3) uint8 frames instead (``decode_latents_uint8``): a quarter of the bytes per
    kept sample, ready for ``image_io.save_frames``.  ``output="jpeg"`` compresses those frames on the decode stream
    (``image_io.JpegEncoder`` at ``jpeg_quality``) and keeps, per sample, one ``list[bytes]`` of F JPEG files for each of its B
    videos, ready for ``image_io.write_avi``: the encoder's buffers are reused, so a sample's bytes are fetched when the next
    sample finishes on this rank (its decode is long over by then) or in ``finish``.  ``output="gif"`` does the same with
    ``image_io.GifEncoder`` at ``gif_fps`` frames per second and keeps, per sample, one ``bytes`` (a complete animated GIF) for
    each of its B videos.  ``output="png"`` mirrors ``"jpeg"`` with ``image_io.PngEncoder``: per sample one ``list[bytes]`` of F PNG
    files (lossless) for each of its B videos; the files are finished on the device (chunks and CRC-32 too) and the fetch only
    copies them.  ``output="webp"`` mirrors ``"gif"`` with ``image_io.WebpEncoder``: per sample one ``bytes`` (a complete
    animated lossless WebP at ``gif_fps`` frames per second) for each of its B videos.

    ``latent_view`` (a callable, default None): applied to a finished latent before it is decoded, for pipelines whose
    carried tensor holds more than the sample -- ``StableVideoUNet(sampler="dpmpp_2m").sample_of`` takes the four sample
    channels out of the 8-channel solver state.

    ``interpolate`` 2 or 4 (default 1: nothing changes) puts motion-compensated frames between each video's frames on the
    decode stream (``image_io.FrameInterpolator`` with ``interp_range`` and ``interp_penalty``) before any of the 8-bit
    outputs: ``"uint8"`` keeps (B, (F-1)*interpolate+1, 8H, 8W, 3), the encoders see that many frames, and ``"gif"`` /
    ``"webp"`` play them at ``gif_fps * interpolate``.  ``output="float32"`` has no 8-bit frames and refuses it.
    """

    def __init__(self, decoder: TemporalDecoderHIP, stage, num_frames: int, *, decode_chunk_size: int = 14,
                 spread: bool = True, keep: str = "all", check_finite: bool = False, output: str = "float32",
                 jpeg_quality: int = 90, gif_fps=7, latent_view=None, interpolate: int = 1, interp_range: int = 16,
                 interp_penalty: int = 4) -> None:
        from ..pipeline.step_assignment import ring_finish_rank

        if latent_view is not None and not callable(latent_view):
            raise ValueError("latent_view must be a callable (finished latent -> the (B,4,F,H,W) latents to decode) or None")
        self.latent_view = latent_view

        if keep not in ("all", "last", "none"):
            raise ValueError("keep must be 'all', 'last' or 'none'")
        if output not in ("float32", "uint8", "jpeg", "gif", "png", "webp"):
            raise ValueError("output must be 'float32', 'uint8', 'jpeg', 'gif', 'png' or 'webp'")
        if check_finite and output != "float32":
            raise ValueError("check_finite needs output='float32' (an 8-bit level cannot show a non-finite value)")
        if output == "jpeg" and not (isinstance(jpeg_quality, int) and 1 <= jpeg_quality <= 100):
            raise ValueError(f"jpeg_quality must be an integer from 1 to 100; got {jpeg_quality!r}")
        if output in ("gif", "webp") and (isinstance(gif_fps, bool) or not isinstance(gif_fps, (int, float)) or not gif_fps > 0):
            raise ValueError(f"gif_fps must be a positive number; got {gif_fps!r}")
        if isinstance(interpolate, bool) or interpolate not in (1, 2, 4):
            raise ValueError(f"interpolate must be 1, 2 or 4; got {interpolate!r}")
        if interpolate > 1 and output == "float32":
            raise ValueError("interpolate works on 8-bit frames: it needs output='uint8', 'jpeg', 'gif', 'png' or 'webp'")
        if interpolate > 1:
            from .image_io import _check_interp_search
            interp_range, interp_penalty = _check_interp_search(interp_range, interp_penalty)
        self.interpolate, self.interp_range, self.interp_penalty = interpolate, interp_range, interp_penalty
        self._interp = None             # the FrameInterpolator, made for the first sample's frame size
        self.output, self.jpeg_quality, self.gif_fps = output, jpeg_quality, gif_fps
        self._play_fps = gif_fps * interpolate if interpolate > 1 else gif_fps      # what the animated outputs are written at
        self._jpeg = None               # the JpegEncoder (or, for output="png", the PngEncoder), made for the first sample's frame size
        self._gif = None                # the GifEncoders (or, for output="webp", the WebpEncoders), one per video of a sample (a video's buffers wait for the fetch)
        self._pending = None            # (sample index, videos, streams or files, lengths, event) of the encode still on the device
        self.decoder, self.stage, self.num_frames = decoder, stage, num_frames
        self.chunk, self.keep, self.check_finite = decode_chunk_size, keep, check_finite
        cfg = stage.config
        self.rank, self.world = cfg.rank, cfg.world_size
        self.ring = bool(cfg.ring and cfg.world_size > 1)
        self.spread = bool(spread and self.ring)         # decodes are spread exactly when the schedule spreads the finishes
        self.device = decoder.device
        self.stream = torch.cuda.Stream(device=self.device)          # decodes
        self._ring_finish_rank = ring_finish_rank
        self.frames: dict[int, torch.Tensor] = {}
        self.stats = {"decoded": 0, "forwarded": 0, "received": 0}   # (forwarded / received stay 0: kept for older readers)
        stage.finished_latent_hook = self._finished
        stage.after_sample_hook = None

    # ---------------------------------------------------------------- who decodes sample i
    def decoder_rank(self, idx: int) -> int:
        """The rank on which sample idx's last step runs."""
        return self._ring_finish_rank(idx, self.world) if self.ring else self.world - 1

    # ---------------------------------------------------------------- hook
    def _finished(self, idx: int, latent: torch.Tensor) -> None:
        """On the rank (and stream) where sample idx's last step was just enqueued."""
        if self.decoder_rank(idx) != self.rank:
            raise RuntimeError(f"sample {idx} finished on rank {self.rank}, the schedule names rank {self.decoder_rank(idx)}")
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        self._decode(idx, latent, ready)

    def _decode(self, idx: int, latent: torch.Tensor, ready) -> None:
        latent.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            if self.latent_view is not None:          # (a view shares the finished latent's storage, recorded above)
                latent = self.latent_view(latent)
            if self.output in ("jpeg", "gif", "png", "webp"):
                self._collect_jpeg()           # before this decode is queued: the encoder's buffers are free again after it
            decode = self.decoder.decode_latents if self.output == "float32" else self.decoder.decode_latents_uint8
            out = decode(latent.contiguous(), self.num_frames, decode_chunk_size=self.chunk)
            if self.interpolate > 1:
                if self._interp is None or (self._interp.height, self._interp.width) != tuple(out.shape[2:4]):
                    from .image_io import FrameInterpolator
                    self._interp = FrameInterpolator(self.device, out.shape[2], out.shape[3], self.interpolate,
                                                     self.interp_range, self.interp_penalty)
                # the interpolator's buffers are reused from video to video, so each result is copied out, in stream
                # order, before the next video's kernels are queued
                videos = out
                out = torch.empty((videos.shape[0], (videos.shape[1] - 1) * self.interpolate + 1, *videos.shape[2:]),
                                  dtype=torch.uint8, device=self.device)
                for kept, video in zip(out, videos):
                    kept.copy_(self._interp(video))
            if self.output in ("jpeg", "png"):
                if self._jpeg is None or (self._jpeg.height, self._jpeg.width) != tuple(out.shape[2:4]):
                    from .image_io import JpegEncoder, PngEncoder
                    self._jpeg = (JpegEncoder(self.device, out.shape[2], out.shape[3], self.jpeg_quality) if self.output == "jpeg"
                                  else PngEncoder(self.device, out.shape[2], out.shape[3]))
                # (a PngEncoder that assembles on the device hands over finished files in place of streams)
                enqueue = self._jpeg.enqueue_files if self._device_files() else self._jpeg.enqueue
                streams, lens = enqueue(out.flatten(0, 1))
                done = torch.cuda.Event()
                done.record(self.stream)
                self._pending = (idx, out.shape[0], streams, lens, done)
            elif self.output in ("gif", "webp"):
                if self._gif is None or len(self._gif) != out.shape[0] or (self._gif[0].height, self._gif[0].width) != tuple(out.shape[2:4]):
                    from .image_io import GifEncoder, WebpEncoder
                    self._gif = [GifEncoder(self.device, out.shape[2], out.shape[3], fps=self._play_fps) if self.output == "gif"
                                 else WebpEncoder(self.device, out.shape[2], out.shape[3]) for _ in range(out.shape[0])]
                bufs = [enc.enqueue(video) for enc, video in zip(self._gif, out)]
                done = torch.cuda.Event()
                done.record(self.stream)
                self._pending = (idx, out.shape[0], bufs, None, done)
        self.stats["decoded"] += 1
        if self.output in ("jpeg", "gif", "png", "webp"):
            return
        self._keep(idx, out)

    def _keep(self, idx: int, out) -> None:
        if self.keep == "all":
            self.frames[idx] = out
        elif self.keep == "last":
            self.frames = {idx: out}

    def _device_files(self) -> bool:
        return self.output == "png" and self._jpeg.assemble == "device"

    def _collect_jpeg(self) -> None:
        if self._pending is None:
            return
        idx, videos, streams, lens, done = self._pending
        self._pending = None
        done.synchronize()
        if self.keep != "none":
            with torch.cuda.stream(self.stream):                      # (the copies queue behind nothing: the stream is idle)
                if self.output == "gif":
                    self._keep(idx, [enc.collect(*bufs) for enc, bufs in zip(self._gif, streams)])
                    return
                if self.output == "webp":
                    from .image_io import write_webp
                    self._keep(idx, [write_webp(None, enc.collect_streams(*bufs), enc.width, enc.height, self._play_fps)
                                     for enc, bufs in zip(self._gif, streams)])
                    return
                files = (self._jpeg.collect_files if self._device_files() else self._jpeg.collect)(streams, lens)
            per = len(files) // videos
            self._keep(idx, [files[v * per:(v + 1) * per] for v in range(videos)])

    # ---------------------------------------------------------------- end of a run
    def finish(self, num_samples: int) -> dict:
        """Wait for this rank's decodes and return ``{sample index: frames}`` for the samples decoded on THIS rank
        (``keep``: all of them, the last one, or none)."""
        self.stream.synchronize()
        self._collect_jpeg()
        if self.check_finite:
            for idx, out in self.frames.items():
                if not bool(torch.isfinite(out).all()):
                    raise FloatingPointError(f"frames of sample {idx} hold non-finite values (fp16 activation range)")
        return self.frames

    def reset(self) -> None:
        """Forget the previous run's bookkeeping (bench.py: warm-up, then the timed region)."""
        self.frames = {}
        self._pending = None
