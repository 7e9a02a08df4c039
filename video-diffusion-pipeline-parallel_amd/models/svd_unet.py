"""``StableVideoUNet`` – the ``model(latent, step)`` adapter of the SVD path, MI355X-native.

API mirror of ``/root/reference/src/models/svd_unet.py`` (same constructor / method names, argument
meaning and errors):

  ``__init__`` ``:42-75``  ``_init_scheduler`` ``:77-102``  ``from_pretrained`` ``:104-164``
  ``init_noise_sigma`` ``:196-199``  ``_default_timestep_schedule`` ``:201-217``
  ``set_conditioning`` ``:219-279``  ``set_dummy_conditioning`` ``:281-338``
  ``clear_conditioning`` ``:340-349``  ``forward`` ``:351-439``

What differs is the execution: ``unet`` is a :class:`SVDUNetHIP` (hand-written gfx950 kernels), the
input scale / concat / permute and the fp32 v-prediction Euler update (+ per-frame CFG mix) are two
fused HIP kernels (``sp_pack_input_f16`` / ``sp_euler_step_f16``), and nothing synchronises the device.
``step`` is an INDEX into the sigma table exactly as in the reference (``svd_unet.py:377-379``), so the
caller decides the order.
"""

from __future__ import annotations

import dataclasses
import math
import os
from collections.abc import Sequence
from dataclasses import dataclass

import torch
import torch.nn as nn

from ..hip import ops
from . import euler_schedule, solver_schedule, tile_plan, window_plan
from .unet_hip import SVDUNetHIP
from .unet_spec import UNetConfig, random_state_dict


@dataclass(frozen=True, eq=False)
class VideoConditioning:
    """Everything one ``StableVideoUNet.forward`` call is conditioned on (``StableVideoUNet.prepare_conditioning``).

    Device tensors, prepared once and never written: ``image_embeddings`` (B,1,D) and ``image_latents`` (B,4,F,H,W)
    fp16; ``added_time_ids`` (B,3) fp16 as the reference builds them; ``added_ids32`` their fp32 form, [3] when every
    video has the same (fps-1, motion bucket, noise aug) triple, else [B][3]; ``guidance32`` None (no guidance), [F]
    (one per-frame scale row for every video, ``guidance_ld`` 0) or [B][F] (one row per video, ``guidance_ld`` = F);
    ``guidance_scale_tensor`` the same scales in fp16, (1 or B, 1, F, 1, 1);
    ``uncond_*`` the zero conditioning of the guidance pass (None without guidance); ``noise_seeds`` int64 [B], each video's
    noise seed for the stochastic samplers (None: none given; ``with_noise_seed``)."""

    image_embeddings: torch.Tensor
    image_latents: torch.Tensor
    added_time_ids: torch.Tensor
    added_ids32: torch.Tensor
    guidance_scale: object
    guidance32: torch.Tensor | None
    guidance_ld: int
    guidance_scale_tensor: torch.Tensor | None
    uncond_embeddings: torch.Tensor | None
    uncond_image_latents: torch.Tensor | None
    num_frames: int
    noise_seeds: torch.Tensor | None = None

    @property
    def guided(self) -> bool:
        return self.guidance32 is not None

    @property
    def batch(self) -> int:
        return self.image_embeddings.shape[0]

    def tensors(self) -> dict:
        """The device tensors by field name (None where absent)."""
        return {k: getattr(self, k) for k in ("image_embeddings", "image_latents", "added_time_ids", "added_ids32",
                                              "guidance32", "guidance_scale_tensor", "uncond_embeddings",
                                              "uncond_image_latents", "noise_seeds")}

    def with_noise_seed(self, seed) -> "VideoConditioning":
        """This conditioning with other noise seeds (one int for every video, or one per video, in [0, 2^63)); every other
        tensor is shared, not copied."""
        return dataclasses.replace(self, noise_seeds=_noise_seeds(seed, self.batch, self.image_embeddings.device))


def _noise_seeds(seed, batch: int, device) -> torch.Tensor | None:
    """``noise_seed=`` of ``prepare_conditioning`` as the int64 [B] device tensor the tails read; None stays None."""
    if seed is None:
        return None
    values = [int(s) for s in _per_video("noise_seed", seed, batch)]
    for s in values:
        if not 0 <= s < 2 ** 63:
            raise ValueError(f"noise_seed must be in [0, 2^63); got {s}")
    return torch.tensor(values, dtype=torch.int64, device=device)


def _per_video(name: str, value, batch: int) -> list:
    """A setting given as a scalar (every video) or as a sequence of one value per video -> list of ``batch`` values."""
    if isinstance(value, torch.Tensor):
        value = value.tolist() if value.dim() else value.item()
    if isinstance(value, (list, tuple)):
        if len(value) != batch:
            raise ValueError(f"{name}: {len(value)} values for a batch of {batch} videos")
        return list(value)
    return [value] * batch


# how a step runs: keywords of ``StableVideoUNet.__init__``, which alone validates them; the class methods pass them on
STEP_OPTIONS = ("sampler", "window_stride", "window_weights", "windows_per_call", "eta", "s_noise", "tile_size", "tile_stride",
                "tile_weights", "batched_cfg")


class StableVideoUNet(nn.Module):
    def __init__(
        self,
        unet,
        timesteps: Sequence[int],
        dtype: torch.dtype = torch.float16,
        num_train_timesteps: int = 1000,
        batched_cfg: bool = False,
        sampler: str = "euler",
        window_stride: int | None = None,
        window_weights: str = "triangle",
        windows_per_call: int = 1,
        eta: float = 1.0,
        s_noise: float = 1.0,
        tile_size=None,
        tile_stride=None,
        tile_weights: str = "triangle",
    ) -> None:
        """``batched_cfg`` (extension): run the unconditional and conditional passes of
        classifier-free guidance as ONE batch-2 UNet forward instead of two sequential passes
        (ref ``svd_unet.py:384-411`` runs them one after the other).

        ``sampler`` (extension; the reference hard-codes Euler, ``svd_unet.py:427-439``): ``"euler"``, or ``"dpmpp_2m"`` for
        DPM-Solver++(2M), second order with still one UNet evaluation per step.  Its history -- the previous step's
        denoised estimate -- rides in the latent: ``forward`` then takes and returns (B,8,F,H,W), channels 0-3 the sample,
        channels 4-7 the estimate (``init_state`` / ``sample_of``), the model keeps no state between calls, and the
        steps are called in index order (0, 1, 2, ...).  ``"euler_a"`` (Euler ancestral, 4-channel latent) and
        ``"dpmpp_2m_sde"`` (the SDE form of 2M, 8-channel state) are the stochastic samplers: every
        step adds fresh noise of scale ``eta`` (0: the deterministic sampler's bytes) times ``s_noise``, evaluated inside
        the tail kernel from the videos' seeds (``prepare_conditioning(..., noise_seed=)``), the step index and the
        element's position -- no generator state, so a sample may change rank, stream or graph lane between steps.  Steps
        ascend as for ``dpmpp_2m``; ``eta`` and ``s_noise`` are ignored by the deterministic samplers.

        ``window_stride`` (extension): long videos by temporal co-denoising.  ``forward`` then accepts a
        latent of more frames than the conditioning's ``num_frames`` = W: every step runs the UNet on overlapping windows of
        W frames, ``window_stride`` apart (``models/window_plan.py``), and ONE sampler update follows behind all windows' eps
        rows, blended per frame with ``window_weights`` ("triangle": a window counts most at its centre; "uniform").
        ``windows_per_call`` windows are stacked as extra batch rows of one UNet call.  None: every path is the unwindowed
        one.

        ``tile_size=(th, tw)``, ``tile_stride=(sy, sx)`` (extension; latent cells): large frames by
        spatial co-denoising.  ``forward`` then accepts a latent whose H x W exceed the tile -- the size the model was trained
        at -- and a conditioning whose ``image_latents`` have the LARGE size: every step runs the UNet on overlapping tiles
        (``models/tile_plan.py``), each conditioned on the crop of the image latents at its own position (the CLIP embedding and
        the added-time ids are shared), and ONE sampler update follows behind all patches' eps rows, blended per pixel with
        the separable ``tile_weights``.  With ``window_stride`` the patches are frame windows times tiles;
        ``windows_per_call`` then counts patches.  None: today's paths."""
        super().__init__()
        if (tile_size is None) != (tile_stride is None):
            raise ValueError(f"tile_size and tile_stride go together (both pairs of latent cells, or both None); got "
                             f"tile_size={tile_size}, tile_stride={tile_stride}")
        if tile_weights not in tile_plan.WEIGHTS:
            raise ValueError(f"tile_weights must be one of {tile_plan.WEIGHTS}; got {tile_weights!r}")
        self.tile_size = self.tile_stride = None
        if tile_size is not None:
            self.tile_size, self.tile_stride = tile_plan._pair("tile_size", tile_size), tile_plan._pair("tile_stride", tile_stride)
            for name, t, st in zip("yx", self.tile_size, self.tile_stride):
                if t < 1 or not 1 <= st <= t:
                    raise ValueError(f"tile plan, {name} (tile={t}, stride={st}): tile must be at least 1 and stride from 1 to tile")
        self.tile_weights = tile_weights
        self._step_plans: dict = {}      # (frames_total, window, H, W) -> ops.TileRecord
        if window_stride is not None and int(window_stride) < 1:
            raise ValueError(f"window_stride must be a positive frame count or None; got {window_stride}")
        if window_weights not in window_plan.WEIGHTS:
            raise ValueError(f"window_weights must be one of {window_plan.WEIGHTS}; got {window_weights!r}")
        if int(windows_per_call) < 1:
            raise ValueError(f"windows_per_call must be at least 1; got {windows_per_call}")
        self.window_stride = None if window_stride is None else int(window_stride)
        self.window_weights = window_weights
        self.windows_per_call = int(windows_per_call)
        if sampler not in solver_schedule.SAMPLERS:
            raise ValueError(f"sampler must be one of {solver_schedule.SAMPLERS}; got {sampler!r}")
        self.sampler = sampler
        self.stochastic = sampler in solver_schedule.STOCHASTIC
        self.eta, self.s_noise = float(eta), float(s_noise)
        self.state_channels = 8 if sampler in ("dpmpp_2m", "dpmpp_2m_sde") else 4
        self.batched_cfg = batched_cfg
        self._use_graphs = os.environ.get("VDPP_GRAPHS", "0") == "1"
        self._graphs: dict = {}          # (calling stream, step, latent shape) -> (graph, static_in, static_out)
        self._graph_lanes: dict = {}     # calling stream -> (capture stream, memory pool) of that lane
        if dtype != torch.float16:
            raise ValueError("the MI355X SVD path computes in float16 (fp32 accumulate)")
        if not isinstance(unet, SVDUNetHIP):
            # any module carrying a diffusers-named UNetSpatioTemporalConditionModel state_dict
            cfg = getattr(unet, "hip_config", None) or UNetConfig.svd()
            device = next(unet.parameters()).device
            unet = SVDUNetHIP(cfg, unet.state_dict(), device)
        self.unet = unet
        self.timesteps = list(timesteps)
        self.dtype = dtype
        self.num_train_timesteps = num_train_timesteps
        self._init_scheduler()
        self._cond: VideoConditioning | None = None      # the model's own conditioning (set_conditioning)
        self._graph_conds: dict = {}     # (calling stream, layout of a VideoConditioning) -> that lane's static copy

    # ------------------------------------------------------------------ schedule
    def _init_scheduler(self) -> None:
        sig = euler_schedule.karras_sigma_table(len(self.timesteps))
        self.sigmas = sig                                   # host fp32 (N+1)
        self.scheduler_timesteps = euler_schedule.continuous_timesteps(sig)
        self._sigma_host = [float(s) for s in sig]
        self._t_dev = self.scheduler_timesteps.to(self.unet.device)   # device table, indexed per step
        self._init_noise_sigma = float((sig[0] ** 2 + 1) ** 0.5)
        self._solver_coef = solver_schedule.dpmpp_2m_coefficients(sig) if self.sampler == "dpmpp_2m" else None
        # the stochastic samplers' per-step constants: (sigma_down, n) / (a, b, c1, c2, n)
        self._noise_coef = None
        if self.sampler == "euler_a":
            self._noise_coef = solver_schedule.euler_ancestral_coefficients(sig, self.eta, self.s_noise)
        elif self.sampler == "dpmpp_2m_sde":
            self._noise_coef = solver_schedule.dpmpp_2m_sde_coefficients(sig, self.eta, self.s_noise)

    # ------------------------------------------------------------------ sampler state
    def init_state(self, noise: torch.Tensor) -> torch.Tensor:
        """The tensor ``forward`` steps, from the initial noise (B,4,F,H,W): the noise itself for Euler; for
        ``dpmpp_2m`` (B,8,F,H,W) with the noise in channels 0-3 and zeros in the history channels (step 0 does not read
        them)."""
        if self.state_channels == 4:
            return noise
        if noise.dim() != 5 or noise.shape[1] != 4:
            raise ValueError(f"noise must be (B, 4, F, H, W); got {tuple(noise.shape)}")
        state = noise.new_zeros((noise.shape[0], 8) + tuple(noise.shape[2:]))
        state[:, :4] = noise
        return state

    def sample_of(self, state: torch.Tensor) -> torch.Tensor:
        """The sample (B,4,F,H,W) inside a stepped tensor: the tensor itself for Euler, a view of channels 0-3 for
        ``dpmpp_2m``."""
        return state if self.state_channels == 4 else state[:, :4]

    def initial_noise(self, seeds, frames: int, h: int, w: int) -> torch.Tensor:
        """The initial latent (B,4,F,H,W) of the videos with the noise seeds ``seeds`` (one int, a sequence of ints or an
        int64 [B] device tensor): ``init_noise_sigma`` times the normals of (seed, step 0, purpose 0, element)
        (``sp_randn_f16``).  A video's noise depends on its seed and shape alone, not on what it is batched with."""
        if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.int64 or not seeds.is_cuda:
            if isinstance(seeds, torch.Tensor):
                seeds = seeds.tolist()
            values = list(seeds) if isinstance(seeds, (list, tuple)) else [seeds]
            seeds = _noise_seeds(values, len(values), self.unet.device)
        out = torch.empty((seeds.shape[0], 4, int(frames), int(h), int(w)), dtype=torch.float16, device=seeds.device)
        return ops.randn(out, seeds.contiguous(), scale=self._init_noise_sigma, step=0, purpose=0)

    @property
    def init_noise_sigma(self) -> float:
        return self._init_noise_sigma

    @staticmethod
    def _default_timestep_schedule(num_steps: int, num_train_timesteps: int = 1000) -> list[int]:
        ratio = num_train_timesteps // num_steps
        return list(range(num_train_timesteps - 1, -1, -ratio))[:num_steps]

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(
        cls,
        model_id: str = "stabilityai/stable-video-diffusion-img2vid-xt",
        timesteps: Sequence[int] | None = None,
        torch_dtype: torch.dtype = torch.float16,
        enable_memory_efficient_attention: bool = True,
        enable_sliced_attention: bool = False,
        attention_slice_size: int | str = "auto",
        device="cuda",
        **kwargs,
    ) -> "StableVideoUNet":
        """Load ``<model_id>/unet/diffusion_pytorch_model*.safetensors`` from a LOCAL directory.

        The attention toggles of the reference signature are accepted and ignored: the fused HIP
        attention kernels are always on.  A hub name cannot be fetched (no network): ValueError.
        Of ``kwargs`` the step options (``STEP_OPTIONS``: ``sampler``, ``window_stride``, ``tile_size``, ...) go to
        ``__init__``, which validates them; the reference's other keywords are accepted and ignored.
        """
        unet_dir = os.path.join(model_id, "unet")
        if not os.path.isdir(unet_dir):
            raise ValueError(
                f"'{model_id}' is not a local model directory; use StableVideoUNet.from_random_init() for "
                "synthetic weights (there is no network access to fetch checkpoints)."
            )
        import json

        from safetensors.torch import load_file

        files = sorted(n for n in os.listdir(unet_dir) if n.endswith(".safetensors"))
        fp16_files = [n for n in files if ".fp16." in n]       # the hub layout ships both variants: read one of them
        sd = {}
        for name in (fp16_files or files):
            sd.update(load_file(os.path.join(unet_dir, name)))
        if not sd:
            raise ValueError(f"no *.safetensors weights under '{unet_dir}'")
        cfg = UNetConfig.svd()
        cfg_path = os.path.join(unet_dir, "config.json")
        if os.path.exists(cfg_path):              # diffusers' UNetSpatioTemporalConditionModel config
            with open(cfg_path) as fh:
                raw = json.load(fh)
            heads = raw.get("num_attention_heads", cfg.num_attention_heads)
            boc = tuple(raw.get("block_out_channels", cfg.block_out_channels))
            if isinstance(heads, int):
                heads = (heads,) * len(boc)
            down_types = raw.get("down_block_types")
            cfg = UNetConfig(
                in_channels=raw.get("in_channels", cfg.in_channels),
                out_channels=raw.get("out_channels", cfg.out_channels),
                block_out_channels=boc,
                layers_per_block=raw.get("layers_per_block", cfg.layers_per_block),
                num_attention_heads=tuple(heads),
                cross_attention_dim=raw.get("cross_attention_dim", cfg.cross_attention_dim),
                addition_time_embed_dim=raw.get("addition_time_embed_dim", cfg.addition_time_embed_dim),
                projection_class_embeddings_input_dim=raw.get("projection_class_embeddings_input_dim",
                                                              cfg.projection_class_embeddings_input_dim),
                down_has_attn=tuple("CrossAttn" in t for t in down_types) if down_types else cfg.down_has_attn,
            )
        if timesteps is None:
            timesteps = cls._default_timestep_schedule(num_steps=25)
        return cls(unet=SVDUNetHIP(cfg, sd, device), timesteps=timesteps, dtype=torch_dtype,
                   **{k: v for k, v in kwargs.items() if k in STEP_OPTIONS})

    @classmethod
    def from_random_init(cls, timesteps: Sequence[int], *, config: UNetConfig | None = None, seed: int = 0,
                         device="cuda", fp8_attention: bool | None = None,
                         long_attention: bool | None = None, **step_options) -> "StableVideoUNet":
        """Random weights of the exact SVD architecture (benchmarks / tests; no checkpoint needed); ``step_options``
        (``STEP_OPTIONS``) as for ``__init__``."""
        unknown = sorted(set(step_options) - set(STEP_OPTIONS))
        if unknown:
            raise TypeError(f"from_random_init() got an unexpected keyword argument {unknown[0]!r}")
        cfg = config or UNetConfig.svd()
        sd = random_state_dict(cfg, seed=seed, device=device, dtype=torch.float16)
        unet = SVDUNetHIP(cfg, sd, device, fp8_attention=fp8_attention, long_attention=long_attention)
        del sd
        return cls(unet=unet, timesteps=timesteps, **step_options)

    def enable_graphs(self, enabled: bool = True) -> None:
        """Replay each diffusion step from a captured HIP graph (one graph per step index and latent shape).

        A step is ~1,100 kernel launches issued from Python; the graph removes that host work from the critical path
        (it matters when the host is slow or the latent is small; at the benchmark shape the GPU is the bottleneck
        either way).  Graphs, their static buffers, their memory pool and the engine's per-stream scratch are all
        private to the HIP stream the caller runs on, so several videos in flight on separate streams
        (``PipelineConfig.concurrent_samples``) never share replay state.  ``set_conditioning`` invalidates them; a
        conditioning passed per call (``forward(..., conditioning=)``) is copied into the lane's static copy of it before
        each replay (one graph per lane, step, latent shape and conditioning layout)."""
        self._use_graphs = enabled
        if not enabled:
            self._drop_replay_state()

    def _drop_replay_state(self) -> None:
        """Forget the captured graphs, their lanes (capture streams / pools are keyed by the calling stream's raw handle), the
        lanes' conditioning copies and the engine's per-stream scratch."""
        self._graphs.clear()
        self._graph_lanes.clear()
        self._graph_conds.clear()
        release = getattr(self.unet, "release_stream_state", None)
        if release is not None:
            release()

    def enable_memory_optimizations(self) -> None:
        """Kept for API compatibility (ref ``svd_unet.py:166-194``); nothing to toggle here."""

    def to(self, *args, **kwargs):  # weights already live on the engine's device
        return self

    # ------------------------------------------------------------------ conditioning
    def prepare_conditioning(
        self,
        image_embeddings: torch.Tensor,
        image_latents: torch.Tensor,
        fps=6,
        motion_bucket_id=127,
        noise_aug_strength=0.02,
        guidance_scale=None,
        num_frames: int = 14,
        noise_seed=None,
    ) -> VideoConditioning:
        """The conditioning of one (micro-)batch of videos as an immutable object for ``forward(..., conditioning=)``.

        ``fps``, ``motion_bucket_id``, ``noise_aug_strength`` and ``guidance_scale`` are each a scalar (every video) or
        a sequence of one value per video.  Guidance of video i is ``linspace(1, g_i, num_frames)`` per frame; a batch
        mixes no guided (g > 1) and unguided videos (ValueError), a sequence of another length than the batch is a
        ValueError.  Videos that agree on all of them run exactly the shared-conditioning path.  ``noise_seed``: one int
        (every video) or one per video, in [0, 2^63): the seeds of the stochastic samplers' noise; None = none."""
        if image_embeddings.dim() == 2:
            image_embeddings = image_embeddings.unsqueeze(1)
        batch = image_embeddings.shape[0]
        dev = self.unet.device
        fps_v = _per_video("fps", fps, batch)
        mb_v = _per_video("motion_bucket_id", motion_bucket_id, batch)
        na_v = _per_video("noise_aug_strength", noise_aug_strength, batch)
        gs_v = _per_video("guidance_scale", guidance_scale, batch)
        guided = [g is not None and g > 1.0 for g in gs_v]
        if any(guided) and not all(guided):
            raise ValueError(f"guidance_scale {gs_v}: a batch cannot mix guided (> 1) and unguided videos "
                             "(the guided ones need an unconditional pass the others do not run)")
        rows = [[f - 1, m, a] for f, m, a in zip(fps_v, mb_v, na_v)]
        host = torch.tensor(rows, dtype=self.dtype)
        if bool((host == host[0]).all()):
            # one triple for the whole batch (ref svd_unet.py:252-259 builds the rows the same way): the engine evaluates
            # the added-time embedding once per call (M = 1); the same device work as for scalar settings
            ids = torch.tensor(rows[:1], dtype=self.dtype, device=dev)
            added = ids.repeat(batch, 1)
            ids32 = ids[0].float().contiguous()
        else:
            added = host.to(dev)
            ids32 = added.float().contiguous()
        emb16 = image_embeddings.to(dev, self.dtype).contiguous()
        lat16 = image_latents.to(dev, self.dtype).contiguous()
        gs16 = g32 = uncond_e = uncond_l = None
        g_ld = 0
        if all(guided):
            uncond_e, uncond_l = torch.zeros_like(emb16), torch.zeros_like(lat16)
            if len(set(float(g) for g in gs_v)) == 1:
                gs16 = torch.linspace(1.0, gs_v[0], num_frames).view(1, 1, num_frames, 1, 1).to(dev, dtype=self.dtype)
                g32 = gs16.flatten().float().contiguous()
            else:                                    # one row of per-frame scales per video
                gs = torch.stack([torch.linspace(1.0, float(g), num_frames) for g in gs_v])
                gs16 = gs.view(batch, 1, num_frames, 1, 1).to(dev, dtype=self.dtype)
                g32 = gs16.reshape(batch, num_frames).float().contiguous()
                g_ld = num_frames
        return VideoConditioning(
            image_embeddings=emb16, image_latents=lat16, added_time_ids=added, added_ids32=ids32,
            guidance_scale=guidance_scale if not isinstance(guidance_scale, (list, torch.Tensor)) else tuple(gs_v),
            guidance32=g32, guidance_ld=g_ld, guidance_scale_tensor=gs16, uncond_embeddings=uncond_e,
            uncond_image_latents=uncond_l, num_frames=int(num_frames), noise_seeds=_noise_seeds(noise_seed, batch, dev))

    def set_conditioning(
        self,
        image_embeddings: torch.Tensor,
        image_latents: torch.Tensor,
        fps: int = 6,
        motion_bucket_id: int = 127,
        noise_aug_strength: float = 0.02,
        guidance_scale: float | None = None,
        num_frames: int = 14,
        noise_seed=None,
    ) -> None:
        self._cond = self.prepare_conditioning(image_embeddings, image_latents, fps=fps, motion_bucket_id=motion_bucket_id,
                                               noise_aug_strength=noise_aug_strength, guidance_scale=guidance_scale,
                                               num_frames=num_frames, noise_seed=noise_seed)
        self._graphs.clear()          # captured graphs hold pointers to the previous conditioning tensors

    def set_dummy_conditioning(
        self,
        batch_size: int,
        num_frames: int,
        height: int,
        width: int,
        device: torch.device,
        fps: int = 6,
        motion_bucket_id: int = 127,
        noise_aug_strength: float = 0.02,
        guidance_scale: float | None = None,
    ) -> None:
        emb = torch.randn(batch_size, 1, self.unet.cfg.cross_attention_dim, device=device, dtype=self.dtype)
        lat = torch.randn(batch_size, 4, num_frames, height, width, device=device, dtype=self.dtype)
        self.set_conditioning(emb, lat, fps=fps, motion_bucket_id=motion_bucket_id,
                              noise_aug_strength=noise_aug_strength, guidance_scale=guidance_scale,
                              num_frames=num_frames)

    @property
    def conditioning(self) -> VideoConditioning | None:
        """The model's own conditioning (``set_conditioning``), e.g. to derive per-sample copies ``with_noise_seed``."""
        return self._cond

    def clear_conditioning(self) -> None:
        self._cond = None
        self._drop_replay_state()

    # ------------------------------------------------------------------ one diffusion step
    def _unet_pass(self, latent, image_latents, embeddings, in_scale, step, euler=None, added_ids32=None, eps_out=None):
        b, _, f, h, w = latent.shape
        rows = torch.empty((b * f * h * w, self.unet.cin_pad), dtype=torch.float16, device=latent.device)
        ops.pack_input(latent, image_latents, rows, in_scale=in_scale, b=b, frames=f, h=h, w=w,
                       cpad=self.unet.cin_pad)
        return self.unet.forward_rows(rows, b=b, frames=f, h=h, w=w, t_value=self._t_dev[step:step + 1],
                                      ctx16=embeddings.reshape(b, -1),
                                      added_ids32=self._cond.added_ids32 if added_ids32 is None else added_ids32, euler=euler,
                                      **({} if eps_out is None else {"eps_out": eps_out}))

    def _unet_passes(self, x, cond: VideoConditioning, step, in_scale, *, eps_out=None, euler=None):
        """The UNet passes of one step on the sample ``x``: the conditional one and, with guidance, the unconditional one,
        as two sequential passes (the reference's order) or, with ``batched_cfg``, as the halves ``[uncond, cond]`` of one
        call.  Returns ``(eps_cond, eps_uncond or None)``.

        ``x`` may hold several patches of all videos stacked as ``[patch][video]`` batch rows, with ``cond`` repeated to match
        (``_patch_conditioning``).  ``eps_out``: ``(rows for eps_cond, rows for eps_uncond or None)`` to store the passes' eps
        rows in (a batched call's halves are copied there).  ``euler``: the Euler tail (``latent``, ``out``, ``sigma``,
        ``sigma_next``) for the epilogue of a sequential conditional pass' last convolution, which applies the guidance mix and
        the update itself: its eps rows never exist in HBM and ``eps_cond`` is None.  A batched call cannot take it: both eps
        come back and the tail is the caller's."""
        ids = cond.added_ids32                                                                # [3], or one row per video
        out_c, out_u = (None, None) if eps_out is None else eps_out
        if not cond.guided:
            return self._unet_pass(x, cond.image_latents, cond.image_embeddings, in_scale, step, euler=euler,
                                   added_ids32=ids, eps_out=out_c), None
        if self.batched_cfg:
            both = self._unet_pass(torch.cat([x, x], dim=0),
                                   torch.cat([cond.uncond_image_latents, cond.image_latents], dim=0),
                                   torch.cat([cond.uncond_embeddings, cond.image_embeddings], dim=0), in_scale, step,
                                   added_ids32=ids if ids.dim() == 1 else torch.cat([ids, ids], dim=0))
            half = both.shape[0] // 2
            eps_u, eps_c = both[:half], both[half:]
            if eps_out is not None:
                eps_u, eps_c = out_u.copy_(eps_u), out_c.copy_(eps_c)
            return eps_c, eps_u
        eps_u = self._unet_pass(x, cond.uncond_image_latents, cond.uncond_embeddings, in_scale, step,
                                added_ids32=ids, eps_out=out_u)
        if euler is not None:
            euler = dict(euler, eps_uncond=eps_u, guidance=cond.guidance32, ld_eps=eps_u.shape[1],
                         ld_guidance=cond.guidance_ld)
        return self._unet_pass(x, cond.image_latents, cond.image_embeddings, in_scale, step, euler=euler,
                               added_ids32=ids, eps_out=out_c), eps_u

    @torch.inference_mode()
    def forward(self, latent: torch.Tensor, step: int, conditioning: VideoConditioning | None = None) -> torch.Tensor:
        """One Euler step of ``latent`` (B,4,F,H,W), or with ``sampler="dpmpp_2m"`` one DPM-Solver++(2M) step of the
        (B,8,F,H,W) state (``init_state``); ``"euler_a"`` / ``"dpmpp_2m_sde"`` step the same tensors and add the step's noise
        from the conditioning's ``noise_seeds``.  ``conditioning`` (``prepare_conditioning``): what this call is conditioned
        on; None = the model's own (``set_conditioning``)."""
        cond = self._cond if conditioning is None else conditioning
        if cond is None:
            raise RuntimeError(
                "Conditioning not set. Call set_conditioning() or set_dummy_conditioning() before forward()."
            )
        if not isinstance(cond, VideoConditioning):
            raise TypeError("conditioning must be a VideoConditioning (StableVideoUNet.prepare_conditioning)")
        if not (0 <= step < len(self.timesteps)):
            raise ValueError(f"Step {step} out of range [0, {len(self.timesteps)})")
        if latent.dtype != torch.float16 or not latent.is_cuda:
            raise ValueError("latent must be a float16 tensor on the HIP device")
        self._check_shapes(latent, cond)
        latent = latent.contiguous()
        if self._use_graphs:
            return self._forward_graph(latent, step, conditioning)
        return self._forward_eager(latent, step, cond)

    def _check_shapes(self, latent: torch.Tensor, cond: VideoConditioning | None = None) -> None:
        """The kernels take raw pointers and the latent's (B, F, H, W): a conditioning tensor of another shape would be
        read out of bounds (the reference fails in ``torch.cat`` / on broadcast, ``svd_unet.py:385-411``)."""
        cond = self._cond if cond is None else cond
        if self.state_channels == 8:
            if latent.dim() == 5 and latent.shape[1] == 4:
                raise ValueError(f"sampler={self.sampler!r} steps a (B, 8, F, H, W) state (sample ++ previous denoised estimate); "
                                 f"got the bare sample {tuple(latent.shape)}: wrap the noise in model.init_state()")
            if latent.dim() != 5 or latent.shape[1] != 8:
                raise ValueError(f"latent must be (B, 8, F, H, W) with sampler={self.sampler!r}; got {tuple(latent.shape)}")
        elif latent.dim() != 5 or latent.shape[1] != 4:
            raise ValueError(f"latent must be (B, 4, F, H, W); got {tuple(latent.shape)}")
        sample_shape = (latent.shape[0], 4) + tuple(latent.shape[2:])
        # with window_stride a long latent against a conditioning prepared for one window of W = num_frames frames
        frames = latent.shape[2] if self.window_stride is None else cond.num_frames
        # ValueError naming (total, tile, stride) of the axis, or (frames_total, window, stride); the plan's tables reach the device here
        self._step_plan(latent.shape[2], frames, latent.shape[3], latent.shape[4])
        if self.window_stride is not None:
            sample_shape = sample_shape[:2] + (frames,) + sample_shape[3:]
            if tuple(cond.image_latents.shape) != sample_shape:
                raise ValueError(f"image_latents {tuple(cond.image_latents.shape)} do not match one window {sample_shape} of "
                                 f"the latent {tuple(latent.shape)} (window_stride={self.window_stride}: the conditioning is "
                                 f"prepared for num_frames = the window length)")
        elif tuple(cond.image_latents.shape) != sample_shape:
            raise ValueError(f"image_latents {tuple(cond.image_latents.shape)} do not match the latent "
                             f"{sample_shape} (set_conditioning was called for another batch / frame count / size)")
        emb = cond.image_embeddings
        if emb.dim() != 3 or emb.shape[0] != latent.shape[0] or emb.shape[1] != 1 \
                or emb.shape[2] != self.unet.cfg.cross_attention_dim:
            raise ValueError(f"image_embeddings must be (B, 1, {self.unet.cfg.cross_attention_dim}) with B = "
                             f"{latent.shape[0]}; got {tuple(emb.shape)}")
        if cond.added_ids32.dim() == 2 and cond.added_ids32.shape[0] != latent.shape[0]:
            raise ValueError(f"added time ids for {cond.added_ids32.shape[0]} videos, the latent has {latent.shape[0]}")
        g = cond.guidance32
        if g is not None and g.shape[-1] != frames:
            raise ValueError(f"guidance was set for num_frames={g.shape[-1]}, the latent has {frames} frames"
                             + (" per window" if self.window_stride is not None else ""))
        if g is not None and g.dim() == 2 and g.shape[0] != latent.shape[0]:
            raise ValueError(f"guidance rows for {g.shape[0]} videos, the latent has {latent.shape[0]}")
        if self.stochastic:
            seeds = cond.noise_seeds
            if seeds is None:
                raise ValueError(f"sampler={self.sampler!r} adds noise at every step and the conditioning carries no seeds: pass "
                                 "noise_seed= to set_conditioning / prepare_conditioning, or use cond.with_noise_seed(seed)")
            if seeds.dtype != torch.int64 or tuple(seeds.shape) != (latent.shape[0],):
                raise ValueError(f"noise_seeds must be int64 [{latent.shape[0]}], one per video of the latent; got "
                                 f"{seeds.dtype} {tuple(seeds.shape)}")

    def _lane_conditioning(self, lane, cond: VideoConditioning):
        """(This lane's static copy of a conditioning of ``cond``'s layout, refreshed from ``cond`` on the calling stream;
        the layout): a graph captured on the copy reads whatever conditioning the lane's current sample has."""
        layout = tuple((k, None if t is None else tuple(t.shape)) for k, t in cond.tensors().items()) + (cond.guidance_ld,)
        static = self._graph_conds.get((lane, layout))
        if static is None:
            static = self._graph_conds[(lane, layout)] = VideoConditioning(
                **{k: (None if t is None else t.clone()) for k, t in cond.tensors().items()},
                guidance_scale=cond.guidance_scale, guidance_ld=cond.guidance_ld, num_frames=cond.num_frames)
        else:
            for k, t in cond.tensors().items():
                if t is not None:
                    getattr(static, k).copy_(t)
        return static, layout

    def _forward_graph(self, latent: torch.Tensor, step: int, conditioning: VideoConditioning | None = None) -> torch.Tensor:
        # Everything a replay touches is keyed by the CALLING stream (one lane of PipelineStage's interleave = one
        # stream): its own graph, static input/output, memory pool, and - because the engine keys its GroupNorm / fp8
        # scratch by the stream it is enqueued on - its own capture stream.  Two lanes replaying at once therefore
        # share nothing but the (read-only) weights and conditioning tensors.  A conditioning passed per call reaches the
        # replay through the lane's static copy of it (one per layout), written on the lane's stream before the replay.
        lane = torch.cuda.current_stream(latent.device).cuda_stream
        key = (lane, step, tuple(latent.shape))
        cond = self._cond
        if conditioning is not None:
            cond, layout = self._lane_conditioning(lane, conditioning)
            key = key + (layout,)
        entry = self._graphs.get(key)
        if entry is None:
            self._forward_eager(latent, step, cond)       # warm-up: lazy allocations, function attributes
            torch.cuda.synchronize(latent.device)
            lane_state = self._graph_lanes.get(lane)
            if lane_state is None:
                lane_state = self._graph_lanes[lane] = [torch.cuda.Stream(device=latent.device), None]
            static_in = latent.clone()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=lane_state[1], stream=lane_state[0]):
                static_out = self._forward_eager(static_in, step, cond)
            if lane_state[1] is None:
                lane_state[1] = graph.pool()
            entry = self._graphs[key] = (graph, static_in, static_out)
        graph, static_in, static_out = entry
        static_in.copy_(latent)
        graph.replay()
        return static_out.clone()                          # the static buffer is overwritten by this lane's next replay

    def _forward_eager(self, latent: torch.Tensor, step: int, cond: VideoConditioning | None = None) -> torch.Tensor:
        cond = self._cond if cond is None else cond
        if self.sampler != "euler" or self.window_stride is not None or self.tile_size is not None:
            return self._forward_stored_eps(latent, step, cond)
        b, _, f, h, w = latent.shape
        sigma, sigma_next = self._sigma_host[step], self._sigma_host[step + 1]
        out = torch.empty_like(latent)
        eps_c, eps_u = self._unet_passes(latent, cond, step, 1.0 / math.sqrt(sigma * sigma + 1.0),
                                         euler=dict(latent=latent, out=out, sigma=sigma, sigma_next=sigma_next))
        if eps_c is not None:                             # the conditional pass did not take the tail
            ops.euler_step(latent, eps_c, eps_u, cond.guidance32 if eps_u is not None else None, out,
                           ld_eps=eps_c.shape[1], sigma=sigma, sigma_next=sigma_next, b=b, frames=f, h=h, w=w,
                           ld_guidance=cond.guidance_ld)
        return out

    # ------------------------------------------------------------------ every other step: stored eps rows, then one tail
    def _step_plan(self, frames_total: int, window: int, h: int, w: int):
        """The ``ops.TileRecord`` (plan, tables on the device) of a latent of ``frames_total`` x ``h`` x ``w`` cut into patches:
        frame windows of ``window`` (``window_stride``; without it one window, the whole video) times tiles of ``tile_size``
        (without it one tile, the whole frame).  None where neither is set: the step is one patch and needs no plan."""
        if self.window_stride is None and self.tile_size is None:
            return None
        key = (int(frames_total), int(window), int(h), int(w))
        rec = self._step_plans.get(key)
        if rec is None:
            size, stride = ((h, w), (h, w)) if self.tile_size is None else (self.tile_size, self.tile_stride)
            pl = tile_plan.plan(h, w, size, stride, self.tile_weights, frames_total=frames_total, window=window,
                                window_stride=window if self.window_stride is None else self.window_stride,
                                window_weights=self.window_weights)
            rec = self._step_plans[key] = ops.TileRecord(pl, self.unet.device, space=self.tile_size is not None)
        return rec

    def _patch_conditioning(self, cond: VideoConditioning, part, th: int, tw: int) -> VideoConditioning:
        """The conditioning of one UNet call on the patches ``part`` stacked as ``[patch][video]`` batch rows: with ``tile_size``
        every patch's crop of the image latents at its own position, without it the image latents themselves; all rows
        repeated per patch."""
        def rep(t):
            return t if len(part) == 1 else torch.cat([t] * len(part), dim=0)

        def crops(t):
            if self.tile_size is None:
                return rep(t)
            return torch.cat([t[:, :, :, y0:y0 + th, x0:x0 + tw] for *_, y0, x0 in part], dim=0).contiguous()

        guided = cond.guided
        return dataclasses.replace(
            cond, image_embeddings=rep(cond.image_embeddings), image_latents=crops(cond.image_latents),
            added_ids32=cond.added_ids32 if cond.added_ids32.dim() == 1 else rep(cond.added_ids32),
            uncond_embeddings=rep(cond.uncond_embeddings) if guided else None,
            uncond_image_latents=crops(cond.uncond_image_latents) if guided else None)

    def _forward_stored_eps(self, state: torch.Tensor, step: int, cond: VideoConditioning) -> torch.Tensor:
        """One step by the stored-eps route: the UNet passes leave their eps rows in HBM and ONE tail kernel follows with this
        step's coefficients (host constants, so a captured graph of the step holds them).  Every sampler but plain Euler takes
        it -- ``conv_out``'s fused Euler epilogue knows neither the solver's history nor the noise -- and so does every step
        with a plan, whose tail must see all patches: a latent of F_total x H x W as n_patch = n_win * n_ty * n_tx patches
        (frame windows of W = ``cond.num_frames`` frames times spatial tiles), the passes on every patch's slice
        (``windows_per_call`` patches of all B videos per call, each conditioned on its own crop), each call's eps rows stored
        to its slice of one [n_patch][B][W][th*tw][4] buffer per pass."""
        b, _, ft, h, w = state.shape
        sigma = self._sigma_host[step]
        in_scale = 1.0 / math.sqrt(sigma * sigma + 1.0)
        win = ft if self.window_stride is None else cond.num_frames
        plan = self._step_plan(ft, win, h, w)
        if plan is None:                                  # (a view for one video; else a copy of the four sample planes)
            x = state[:, :4].contiguous() if self.state_channels == 8 else state
            eps_c, eps_u = self._unet_passes(x, cond, step, in_scale)
        else:
            x = self.sample_of(state)
            th, tw = plan.plan.tile
            patches = plan.plan.patches()
            rows = b * win * th * tw                          # eps rows of one patch of all videos
            eps_c = torch.empty((len(patches) * rows, self.unet.cfg.out_channels), dtype=torch.float16, device=state.device)
            eps_u = torch.empty_like(eps_c) if cond.guided else None
            for k0 in range(0, len(patches), self.windows_per_call):
                part = patches[k0:k0 + self.windows_per_call]
                # [patch][video] batch rows: the layout of the eps buffer
                xs = torch.cat([x[:, :, f0:f0 + win, y0:y0 + th, x0:x0 + tw] for _, _, _, f0, y0, x0 in part], dim=0).contiguous()
                dst = slice(k0 * rows, (k0 + len(part)) * rows)
                self._unet_passes(xs, self._patch_conditioning(cond, part, th, tw), step, in_scale,
                                  eps_out=(eps_c[dst], eps_u[dst] if cond.guided else None))
        return self._tail(state, eps_c, eps_u, torch.empty_like(state), step, cond, plan)

    def _tail(self, state, eps_c, eps_u, out, step: int, cond: VideoConditioning, plan) -> torch.Tensor:
        """The sampler update of ``state`` into ``out`` behind the stored eps rows.  The sampler gives the step's constants; what
        the model was configured with gives the entry: the tiles entries with ``tile_size``; else the stochastic entries, with
        the window arguments where ``window_stride`` is set; else the windows entries; else the rows entries."""
        b, _, ft, h, w = state.shape
        solver = self.state_channels == 8
        if solver:                                        # (a, b, c1, c2), with noise (a, b, c1, c2, n)
            coef = (self._noise_coef if self.stochastic else self._solver_coef)[step]
            consts = dict(a=coef[0], b=coef[1], c1=coef[2], c2=coef[3], batch=b)
        else:                                             # the sigma the Euler step goes to; with noise (sigma_down, n)
            coef = self._noise_coef[step] if self.stochastic else (self._sigma_host[step + 1],)
            sigma_to, consts = coef[0], dict(b=b)
        # the noise of element (f, y, x), whichever patches cover it
        noise = dict(noise_scale=coef[-1], seeds=cond.noise_seeds, step=step) if self.stochastic else {}
        args = (state, eps_c, eps_u, cond.guidance32 if eps_u is not None else None, out)
        kw = dict(ld_eps=eps_c.shape[1], sigma=self._sigma_host[step], ld_guidance=cond.guidance_ld, **consts, **noise)
        if self.tile_size is not None:
            if solver:
                return ops.dpmpp2m_step_tiles(*args, plan=plan, **kw)
            return ops.euler_step_tiles(*args, plan=plan, sigma_next=sigma_to, **kw)
        kw.update(h=h, w=w)
        if plan is not None:                              # window_stride alone: the frame half of the plan as arguments
            fr = plan.plan.frames
            kw.update(window=fr.window, stride=fr.stride, n_win=fr.n_win, weights=plan.wf)
        if self.stochastic:
            if solver:
                return ops.dpmpp2m_sde_step(*args, frames_total=ft, **kw)
            return ops.euler_ancestral_step(*args, frames_total=ft, sigma_down=sigma_to, **kw)
        if plan is not None:
            if solver:
                return ops.dpmpp2m_step_windows(*args, frames_total=ft, **kw)
            return ops.euler_step_windows(*args, frames_total=ft, sigma_next=sigma_to, **kw)
        if solver:
            return ops.dpmpp2m_step(*args, frames=ft, **kw)
        return ops.euler_step(*args, frames=ft, sigma_next=sigma_to, **kw)
