"""Can the whole-model parity tests of the three edge engines see their attention, their temporal half and their ends?
Helpers for tests/test_edge_sensitivity_cpu.py and tests/test_edge_peaked_gpu.py (plain module: no fixtures, no tests;
``python -m tests.edge_mutants`` prints the table kept in profiles/edge_sensitivity.txt).  The UNet's counterpart is
tests/unet_mutants.py, whose ``fp16_storage``, ``rel_l2``, ``FACTOR`` and ``MARGIN`` are used here as they are.

* ``peaked_decoder_state_dict`` / ``peaked_encoder_state_dict`` / ``peaked_clip_state_dict``  the project's random weights
  with the attention Q/K projections scaled up (and V / out scaled), so that every softmax row has a dominant key; the
  decoder's ``time_mixer.mix_factor`` set away from 0 with mixed signs and magnitudes.  Rounded to fp16 afterwards.
* ``MUTANTS``  plausible bugs of ``TemporalDecoderHIP`` / ``ImageEncoderHIP`` / ``CLIPVisionHIP``, applied to the ORACLE
  at run time (context manager ``mutate``; oracle/ is not edited), everywhere or in one named block.
* ``capture_oracle`` / ``capture_engine``  input and output of every block as [rows][C], in call order: forward hooks on
  the oracle's ``SpatioTemporalResBlock`` / ``_Attention`` / top-level ``_Res2D`` (CLIP: ``output_hidden_states=True``,
  all tokens) and wrappers around ``_run_res`` / ``_run_attn`` / ``_run_res2d`` / ``_run_layer`` of the engine instance.
* ``noise_and_bounds``  the fp32 oracle and its fp16-storage emulation on the same inputs: the noise floor a bound for the
  engine is derived from (``T = FACTOR x noise``, per quantity).  Nothing in it comes from an engine.
"""
from __future__ import annotations

import contextlib
import functools
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import vae_temporal_decoder_ref as V
from tests.unet_mutants import FACTOR, MARGIN, fp16_storage, rel_l2  # noqa: F401  (the project's own, not forked)

SEED = 3


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    model: str            # "decoder" | "encoder" | "clip"
    kind: str             # decoder: "decode" | "latents"; encoder: "encode"; clip: "small" | "vith"
    b: int = 1            # items of a decode call / videos / images
    f: int = 1            # frames per item or video
    h: int = 0            # latent height (decoder), image height (encoder)
    w: int = 0
    chunk: int = 0        # decode_chunk_size of a "latents" case

    @property
    def oracle_key(self):
        return self.model if self.model != "clip" else "clip-" + self.kind


# the shapes of the GPU test and of the CPU sensitivity table: the smallest at which each route can go wrong
CASES = {c.name: c for c in (
    Case("decode 1x4x8x16", "decoder", "decode", 1, 4, 8, 16),          # 128 tokens a frame: fp16-score route
    Case("decode 1x3x16x16", "decoder", "decode", 1, 3, 16, 16),        # 256 tokens: the smallest fp32-score frame
    Case("decode 2x3x8x8", "decoder", "decode", 2, 3, 8, 8),            # two items in one call
    Case("latents 2x3x8x8 chunk 4", "decoder", "latents", 2, 3, 8, 8, 4),     # chunks (4, 2) straddle the videos
    Case("latents 2x3x8x8 chunk 14", "decoder", "latents", 2, 3, 8, 8, 14),   # one call: six frames as one item
    Case("encode 2x64x128", "encoder", "encode", 2, 1, 64, 128),        # 128 tokens
    Case("encode 2x128x128", "encoder", "encode", 2, 1, 128, 128),      # 256 tokens
    Case("clip small 2x56", "clip", "small", 2),                        # 128 wide, 2 heads of 64, 3 layers, 17 tokens
    Case("clip vit-h/14 2 layers 2x224", "clip", "vith", 2),            # 1280 wide, 16 heads of 80, 257 tokens, gelu
)}
ENCODE_FRAMES = 2         # encode_image_latents repeats the latent over this many frames


def clip_config(kind):
    from transformers import CLIPVisionConfig
    if kind == "small":
        return CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2,
                                image_size=56, patch_size=14, projection_dim=64, hidden_act="quick_gelu")
    return CLIPVisionConfig(hidden_size=1280, intermediate_size=5120, num_hidden_layers=2 if kind == "vith" else 4,
                            num_attention_heads=16, image_size=224, patch_size=14, projection_dim=1024, hidden_act="gelu")


# ------------------------------------------------------------------------------------------------ weights
_MIX = (1.5, -1.5, 1.0, -2.0, 2.0, -1.0)      # sigmoid: 0.82 0.18 0.73 0.12 0.88 0.27 -- cycled over the 14 blocks


def _scaled(sd, gains, expect):
    hit = 0
    for name in sd:
        for tail, gain in gains.items():
            if name.endswith(tail):
                sd[name] = sd[name] * gain
                hit += 1
    assert hit == expect, f"{hit} attention parameters scaled, expected {expect}"
    return sd


def peaked_decoder_state_dict(cfg, seed=SEED, qk_gain=4.0, v_gain=2.0, vb_gain=4.0, dtype=torch.float16):
    """``vae_hip.random_state_dict`` with the mid attention's ``to_q`` / ``to_k`` weights x ``qk_gain`` (logits x
    qk_gain^2), ``to_v.weight`` x ``v_gain``, ``to_v.bias`` x ``vb_gain`` and every ``time_mixer.mix_factor`` replaced
    by the next of (1.5, -1.5, 1, -2, 2, -1): the blend weights are 0.12 ... 0.88, neither symmetric nor the same in any
    two neighbouring blocks.  Tuning (CPU, tiny(64), 4 x 8 x 16; all figures in profiles/edge_sensitivity.txt): under
    the plain weights the logits have a standard deviation of 0.33, the largest probability of a row is 0.018 against
    1/128 and the attention branch is 0.15 of its input; gain 4 gives 5.2, 0.66 and 0.87, with a largest |logit| of 39
    (fp16 spacing 0.03 on the fp16-score route, which is as far as that route should be asked to go: no higher gain).
    ``to_v.bias`` is U(+-1/16), a standard deviation of 0.035 against values of 1.2: with ``vb_gain`` 1 a dropped or
    doubled value bias moves the final output by 3.4 x its bound, with 4 by 14 x."""
    from vdpp_amd.models.vae_hip import random_state_dict
    sd = random_state_dict(cfg, seed=seed, dtype=torch.float32)
    a = "mid_block.attentions.0"
    _scaled(sd, {a + ".to_q.weight": qk_gain, a + ".to_k.weight": qk_gain, a + ".to_v.weight": v_gain,
                 a + ".to_v.bias": vb_gain}, 4)
    mixers = [k for k in sd if k.endswith("time_mixer.mix_factor")]
    assert len(mixers) == 14
    for i, k in enumerate(mixers):
        sd[k] = torch.full_like(sd[k], _MIX[i % len(_MIX)])
    return {k: v.to(dtype) for k, v in sd.items()}


def peaked_encoder_state_dict(cfg, seed=SEED, qk_gain=4.0, v_gain=2.0, vb_gain=4.0, dtype=torch.float16):
    """``vae_hip.random_encoder_state_dict`` with the same gains on the encoder's mid attention as the decoder's."""
    from vdpp_amd.models.vae_hip import random_encoder_state_dict
    sd = random_encoder_state_dict(cfg, seed=seed, dtype=torch.float32)
    a = "encoder.mid_block.attentions.0"
    _scaled(sd, {a + ".to_q.weight": qk_gain, a + ".to_k.weight": qk_gain, a + ".to_v.weight": v_gain,
                 a + ".to_v.bias": vb_gain}, 4)
    return {k: v.to(dtype) for k, v in sd.items()}


def plain_clip_model(cfg):
    """The recipe of ``tests/test_clip_gpu.py::_pair``: transformers' own initialisation under seed 1234, biases and norm
    parameters perturbed by 0.1 N(0, 1) under seed 5, everything rounded to fp16."""
    from transformers import CLIPVisionModelWithProjection
    with torch.random.fork_rng():
        torch.manual_seed(1234)
        ref = CLIPVisionModelWithProjection(cfg).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name.endswith("bias") or "norm" in name or "layrnorm" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for p in ref.parameters():
            p.copy_(p.half().float())
    return ref


def peaked_clip_state_dict(cfg, qk_gain=None, v_gain=2.0, fc2_gain=3.0, dtype=torch.float16):
    """The ``_pair`` recipe with every layer's ``q_proj`` / ``k_proj`` (weight and bias) x ``qk_gain``, ``v_proj``
    x ``v_gain`` and ``mlp.fc2.weight`` x ``fc2_gain``.  transformers initialises the projections with a standard
    deviation of 1 / sqrt(2 C layers): the plain logits of a four-layer ViT-H/14 have a standard deviation of 0.14.
    ``qk_gain`` None takes 4.5 for the 128-wide configuration and 3.5 for the 1280-wide one, which puts the logits of
    both at 3.2 to 3.9.  ``fc2_gain`` is there for one mutant: gelu and quick_gelu differ by 3 % of the MLP's output at most,
    and at gain 1 the swap moves a layer's branch by 1.2 to 2.4 x its bound and image_embeds by 1.97 x; at 3 the MLP
    weighs more in the branch and the figures are 2.5 to 4.7 x (a dropped key, the next weakest, keeps 5.6 x at 257
    keys)."""
    if qk_gain is None:
        qk_gain = 4.5 if cfg.hidden_size == 128 else 3.5
    sd = {k: v.clone() for k, v in plain_clip_model(cfg).state_dict().items()}
    gains = {".mlp.fc2.weight": fc2_gain}
    for n, gain in (("q_proj", qk_gain), ("k_proj", qk_gain), ("v_proj", v_gain)):
        gains[f".self_attn.{n}.weight"] = gains[f".self_attn.{n}.bias"] = gain
    _scaled(sd, gains, 7 * cfg.num_hidden_layers)
    return {k: v.to(dtype) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ oracles, inputs
def vae_configs(c=64):
    from vdpp_amd.models.vae_hip import VAEDecoderConfig
    return VAEDecoderConfig.tiny(c), V.VAEDecoderConfig.tiny(c)


def peaked_state_dict(case: Case):
    if case.model == "decoder":
        return peaked_decoder_state_dict(vae_configs()[0])
    if case.model == "encoder":
        return peaked_encoder_state_dict(vae_configs()[0])
    return peaked_clip_state_dict(clip_config(case.kind))


def build_oracle(case: Case, sd):
    if case.model == "clip":
        from transformers import CLIPVisionModelWithProjection
        with torch.random.fork_rng():
            ref = CLIPVisionModelWithProjection(clip_config(case.kind)).eval()
    else:
        ref = (V.TemporalDecoderRef if case.model == "decoder" else V.EncoderRef)(vae_configs()[1]).eval()
    ref.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return ref


@functools.lru_cache(maxsize=None)
def peaked_oracle(key):
    case = next(c for c in CASES.values() if c.oracle_key == key)
    return build_oracle(case, peaked_state_dict(case))


def case_inputs(case: Case):
    """The fp16-rounded input of a case.  Items, videos and images of a call differ in content and in scale."""
    g = torch.Generator().manual_seed(11 + case.h + case.f + case.chunk)
    if case.model == "decoder":
        if case.kind == "decode":
            x = torch.randn(case.b, case.f, 4, case.h, case.w, generator=g)
        else:
            x = torch.randn(case.b, 4, case.f, case.h, case.w, generator=g) * vae_configs()[0].scaling_factor
    elif case.model == "encoder":
        x = torch.randn(case.b, 3, case.h, case.w, generator=g).clamp(-1.5, 1.5)
    else:
        size = clip_config(case.kind).image_size
        x = torch.randn(case.b, 3, size, size, generator=g)
    if case.b > 1:
        x[1] *= 1.7
    if case.model == "decoder" and case.kind == "decode":
        x = x.flatten(0, 1)
    return x.half()


def _decode_latents_per_video(latents, decoder, num_frames, decode_chunk_size):
    """MUTANT of ``oracle.decode_latents``: the chunks are cut inside each video instead of over the flattened (B, F)
    list, so no decoder call straddles two videos."""
    sf = decoder.cfg.scaling_factor
    vids = []
    for v in latents.permute(0, 2, 1, 3, 4) / sf:
        vids.append(torch.cat([decoder(v[i:i + decode_chunk_size], v[i:i + decode_chunk_size].shape[0])
                               for i in range(0, num_frames, decode_chunk_size)]))
    return torch.stack(vids).permute(0, 2, 1, 3, 4).float()


def run_oracle(ref, case: Case, x):
    """The compared output of a case: decode -> (B*F, 3, 8H, 8W); latents -> (B, 3, F, 8H, 8W); encode ->
    (B, 4, ENCODE_FRAMES, H/8, W/8); clip -> image_embeds (B, projection)."""
    with torch.no_grad():
        if case.model == "decoder" and case.kind == "decode":
            return ref(x.float(), case.f)
        if case.model == "decoder":
            fn = _decode_latents_per_video if ref.__dict__.get("_chunks_per_video") else V.decode_latents
            return fn(x.float(), ref, case.f, case.chunk)
        if case.model == "encoder":
            return V.encode_image_latents(x.float(), ref, ENCODE_FRAMES)
        return ref(pixel_values=x.float()).image_embeds


def run_engine(hip, case: Case, x):
    """The same quantity from the HIP engine, ``x`` already on its device."""
    if case.model == "decoder" and case.kind == "decode":
        return hip.decode(x, case.f)
    if case.model == "decoder":
        return hip.decode_latents(x, case.f, decode_chunk_size=case.chunk)
    if case.model == "encoder":
        return hip.encode_image_latents(x, ENCODE_FRAMES)
    return hip(x)


# ------------------------------------------------------------------------------------------------ block capture
@dataclass
class Block:
    name: str             # the oracle's module path; engine side: "" (matched by position)
    kind: str             # "res" (SpatioTemporalResBlock) | "res2d" | "attn" | "layer" (CLIP encoder layer)
    x: torch.Tensor       # input  [rows][Cin]
    y: torch.Tensor       # output [rows][C]
    args: tuple = None    # oracle side, on request: the module's own arguments (to run the block alone)

    @property
    def branch(self):
        """What the block adds to its input; a resnet that changes the width has no identity path: its output."""
        return self.y.float() - self.x.float() if self.x.shape == self.y.shape else self.y.float()


def _rows(t):             # (N, C, H, W) -> [rows][C] in (image, y, x) order; (B, tokens, C) -> [rows][C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t.reshape(-1, t.shape[-1])


def _block_kind(name, m):
    if isinstance(m, V.SpatioTemporalResBlock):
        return "res"
    if isinstance(m, V._Attention):
        return "attn"
    if isinstance(m, V._Res2D) and "spatial_res_block" not in name:      # the encoder's own resnets
        return "res2d"
    return None


def _is_clip(ref):
    return hasattr(ref, "vision_model")


@contextlib.contextmanager
def capture_oracle(oracle, keep_args=False):
    rec, hooks = [], []
    if _is_clip(oracle):
        layers = oracle.vision_model.encoder.layers

        def collect(mod, args, kwargs, out):
            hs = out.hidden_states
            assert hs is not None and len(hs) == len(layers) + 1
            for i in range(len(layers)):
                rec.append(Block(f"vision_model.encoder.layers.{i}", "layer", _rows(hs[i]).clone(), _rows(hs[i + 1]).clone(),
                                 (hs[i], None) if keep_args else None))
        hooks.append(oracle.register_forward_pre_hook(lambda mod, args, kwargs: (args, dict(kwargs, output_hidden_states=True)),
                                                      with_kwargs=True))
        hooks.append(oracle.register_forward_hook(collect, with_kwargs=True))
    for name, m in oracle.named_modules():
        kind = _block_kind(name, m)
        if kind is None:
            continue

        def hook(mod, args, out, name=name, kind=kind):
            rec.append(Block(name, kind, _rows(args[0]).clone(), _rows(out).clone(), args if keep_args else None))
        hooks.append(m.register_forward_hook(hook))
    try:
        yield rec
    finally:
        for h in hooks:
            h.remove()


@contextlib.contextmanager
def capture_engine(hip):
    """Wraps ``_run_res`` / ``_run_attn`` (decoder), ``_run_res2d`` / ``_run_attn`` (encoder) or ``_run_layer`` (CLIP) of
    this instance.  Input and output are cloned at once: the views live in recycled buffers, and a clone on the same
    stream is ordered behind the producer.  The encoder engine works on the image mirrored in both axes, which in rows is
    the reversed token order of every image: its blocks are turned back here."""
    rec = []
    mirrored = type(hip).__name__ == "ImageEncoderHIP"

    def rows(t, n):
        return t.reshape(n, -1, t.shape[1]).flip(1).reshape(t.shape) if mirrored else t.clone()

    def wrap(kind, orig, act):
        @functools.wraps(orig)
        def run(p, x, n, *a, **kw):
            xin = rows(x.t if act else x, n)
            y = orig(p, x, n, *a, **kw)
            rec.append(Block("", kind, xin, rows(y.t if act else y, n)))
            return y
        return run

    names = [(n, k) for n, k in (("_run_res", "res"), ("_run_res2d", "res2d"), ("_run_attn", "attn"), ("_run_layer", "layer"))
             if hasattr(hip, n)]
    for n, k in names:
        setattr(hip, n, wrap(k, getattr(hip, n), k != "layer"))
    try:
        yield rec
    finally:
        for n, _ in names:
            delattr(hip, n)


def assert_same_blocks(engine, oracle):
    assert [b.kind for b in engine] == [b.kind for b in oracle], "engine and oracle ran different block sequences"
    for e, o in zip(engine, oracle):
        assert e.x.shape == o.x.shape and e.y.shape == o.y.shape, f"{o.name}: {tuple(e.x.shape)} -> {tuple(e.y.shape)} " \
            f"against the oracle's {tuple(o.x.shape)} -> {tuple(o.y.shape)}"


# ------------------------------------------------------------------------------------------------ mutants
@dataclass(frozen=True)
class Mutant:
    name: str
    family: str           # "vae_attn" | "dec_res" | "dec_end" | "enc_end" | "clip_attn" | "clip_end"
    what: str
    drop_key: bool = False

    @property
    def in_block(self):   # acts inside a captured block, so that it can be planted in one block alone
        return self.family in ("vae_attn", "dec_res", "clip_attn") or self.what == "act"


MUTANTS = (
    Mutant("vae attention: softmax -> mean of V", "vae_attn", "mean"),
    Mutant("vae attention: logits x2", "vae_attn", "scale2"),
    Mutant("vae attention: 1/sqrt(C) omitted", "vae_attn", "noscale"),
    Mutant("vae attention: last key dropped", "vae_attn", "dropkey", drop_key=True),
    Mutant("vae attention: S transposed", "vae_attn", "transpose"),
    Mutant("vae attention: K/V of the neighbouring frame", "vae_attn", "frame"),
    Mutant("vae attention: to_v bias dropped", "vae_attn", "vbias0"),
    Mutant("vae attention: to_v bias added twice", "vae_attn", "vbias2"),
    Mutant("resblock: blend operands swapped", "dec_res", "blend"),
    Mutant("resblock: temporal taps reversed", "dec_res", "taps"),
    Mutant("resblock: temporal conv wraps round", "dec_res", "wrap"),
    Mutant("resblock: temporal half across items", "dec_res", "items"),
    Mutant("resblock: temporal GroupNorm per frame", "dec_res", "gnframe"),
    Mutant("resblock: conv_shortcut skipped", "dec_res", "noshortcut"),
    Mutant("decoder: upsampling gathered one pixel off", "dec_end", "upsample"),
    Mutant("decoder: time_conv_out taps reversed", "dec_end", "tco_taps"),
    Mutant("decoder: time_conv_out across items", "dec_end", "tco_items"),
    Mutant("decoder: chunks cut per video", "dec_end", "chunks"),
    Mutant("encoder: stride-2 padding top/left", "enc_end", "padtl"),
    Mutant("encoder: logvar half taken as the mode", "enc_end", "half"),
    Mutant("clip: softmax -> mean of V", "clip_attn", "mean"),
    Mutant("clip: scale x2", "clip_attn", "scale2"),
    Mutant("clip: last key dropped", "clip_attn", "dropkey", drop_key=True),
    Mutant("clip: K/V heads rotated by one", "clip_attn", "heads"),
    Mutant("clip: K/V of the other image", "clip_attn", "image"),
    Mutant("clip: position rows shifted by one", "clip_end", "pos"),
    Mutant("clip: pre_layrnorm dropped", "clip_end", "preln"),
    Mutant("clip: gelu <-> quick_gelu", "clip_end", "act"),
    Mutant("clip: pooled taken from token 1", "clip_end", "pooled"),
)


def by_name(name) -> Mutant:
    return next(m for m in MUTANTS if m.name == name)


def engines(mut: Mutant) -> tuple:
    return {"vae_attn": ("decoder", "encoder"), "dec_res": ("decoder",), "dec_end": ("decoder",), "enc_end": ("encoder",),
            "clip_attn": ("clip",), "clip_end": ("clip",)}[mut.family]


def applies(mut: Mutant, case: Case) -> bool:
    """Whether the mutant can change anything in this case at all.  The documented exceptions: a decoder call of ONE item
    has nothing to run across ("across items": every case but ``decode 2x3x8x8``; ``decode_latents`` always calls with
    one item), and only ``decode_latents`` cuts chunks."""
    if case.model not in engines(mut):
        return False
    if mut.what in ("items", "tco_items"):
        return case.kind == "decode" and case.b > 1
    if mut.what == "chunks":
        return case.kind == "latents"
    return True


def _vae_attention(att, what, x):
    """``oracle._Attention.forward`` with one thing wrong."""
    n, c, h, w = x.shape
    t = att.group_norm(x.reshape(n, c, h * w)).transpose(1, 2)
    q, k, v = att.to_q(t), att.to_k(t), att.to_v(t)
    if what == "frame":
        k, v = k.roll(1, dims=0), v.roll(1, dims=0)
    if what == "vbias0":
        v = v - att.to_v.bias
    if what == "vbias2":
        v = v + att.to_v.bias
    if what == "dropkey":
        k, v = k[:, :-1], v[:, :-1]
    if what == "mean":
        o = v.mean(dim=1, keepdim=True).expand_as(q)
    else:
        s = q @ k.transpose(1, 2)
        if what == "transpose":
            s = s.transpose(1, 2)
        s = s * {"scale2": 2.0 / math.sqrt(c), "noscale": 1.0}.get(what, 1.0 / math.sqrt(c))
        o = torch.softmax(s, dim=-1) @ v
    return x + att.to_out[0](o).transpose(1, 2).reshape(n, c, h, w)


def _res_block(blk, what, x, frames):
    """``oracle.SpatioTemporalResBlock.forward`` with one thing wrong."""
    sp, tp = blk.spatial_res_block, blk.temporal_res_block
    if what == "noshortcut" and sp.conv_shortcut is not None:       # the identity on the channels both sides have
        hh = sp.conv2(F.silu(sp.norm2(sp.conv1(F.silu(sp.norm1(x))))))
        s = x[:, :hh.shape[1]] + hh
    else:
        s = sp(x)
    bf, c, h, w = s.shape
    s5 = s.reshape(bf // frames, frames, c, h, w).permute(0, 2, 1, 3, 4)
    z = s5.permute(1, 0, 2, 3, 4).reshape(1, c, bf, h, w) if what == "items" else s5

    def norm(n, t):
        if what != "gnframe":
            return n(t)
        b_, c_, f_, h_, w_ = t.shape
        u = F.group_norm(t.permute(0, 2, 1, 3, 4).reshape(b_ * f_, c_, h_, w_), n.num_groups, n.weight, n.bias, n.eps)
        return u.reshape(b_, f_, c_, h_, w_).permute(0, 2, 1, 3, 4)

    def conv(cv, t):
        if what == "taps":
            return F.conv3d(t, cv.weight.flip(2), cv.bias, padding=(1, 0, 0))
        if what == "wrap":
            return F.conv3d(F.pad(t, (0, 0, 0, 0, 1, 1), mode="circular"), cv.weight, cv.bias)
        return cv(t)

    hh = conv(tp.conv1, F.silu(norm(tp.norm1, z)))
    t5 = z + conv(tp.conv2, F.silu(norm(tp.norm2, hh)))
    if what == "items":
        t5 = t5.reshape(c, bf // frames, frames, h, w).permute(1, 0, 2, 3, 4)
    alpha = 1.0 - torch.sigmoid(blk.time_mixer.mix_factor).to(s.dtype)
    if what == "blend":
        alpha = 1.0 - alpha
    out = alpha * s5 + (1.0 - alpha) * t5
    return out.permute(0, 2, 1, 3, 4).reshape(bf, c, h, w)


def _clip_attention(att, what, hidden_states, attention_mask=None, **kw):
    """``transformers`` ``CLIPAttention.forward`` with one thing wrong."""
    x = hidden_states
    b, n, _ = x.shape
    ctx = x.flip(0) if what == "image" else x
    q, k, v = [p(t).view(b, n, att.num_heads, att.head_dim).transpose(1, 2)
               for p, t in ((att.q_proj, x), (att.k_proj, ctx), (att.v_proj, ctx))]
    if what == "heads":
        k, v = k.roll(1, dims=1), v.roll(1, dims=1)
    if what == "dropkey":
        k, v = k[:, :, :-1], v[:, :, :-1]
    if what == "mean":
        o = v.mean(dim=2, keepdim=True).expand_as(q)
    else:
        o = F.scaled_dot_product_attention(q, k, v, scale=att.scale * (2.0 if what == "scale2" else 1.0))
    return att.out_proj(o.transpose(1, 2).reshape(b, n, -1)), None


def _patch(mod, fn, undo):
    mod.forward = fn          # an instance attribute in front of the class's forward: removed again by undo
    undo.append(lambda: mod.__delattr__("forward"))


def _apply_model(mut: Mutant, ref, undo):
    """The mutants that sit outside the captured blocks."""
    what = mut.what
    if what == "upsample":                          # source pixel (i + 1) // 2 instead of i // 2, in both axes
        for m in [m for m in ref.modules() if isinstance(m, V._Upsample)]:
            def up(x, m=m):
                iy = ((torch.arange(2 * x.shape[2]) + 1) // 2).clamp(max=x.shape[2] - 1)
                ix = ((torch.arange(2 * x.shape[3]) + 1) // 2).clamp(max=x.shape[3] - 1)
                return m.conv(x[:, :, iy][:, :, :, ix])
            _patch(m, up, undo)
    elif what in ("tco_taps", "tco_items"):
        tco = ref.time_conv_out

        def out(x5):                                # (B, 3, F, H, W)
            if what == "tco_taps":
                return F.conv3d(x5, tco.weight.flip(2), tco.bias, padding=(1, 0, 0))
            b, c, f, h, w = x5.shape
            y = F.conv3d(x5.permute(1, 0, 2, 3, 4).reshape(1, c, b * f, h, w), tco.weight, tco.bias, padding=(1, 0, 0))
            return y.reshape(c, b, f, h, w).permute(1, 0, 2, 3, 4)
        _patch(tco, out, undo)
    elif what == "chunks":
        ref._chunks_per_video = True                # read by run_oracle
        undo.append(lambda: ref.__delattr__("_chunks_per_video"))
    elif what == "padtl":
        for m in [m for m in ref.modules() if isinstance(m, V._Downsample)]:
            _patch(m, lambda x, m=m: m.conv(F.pad(x, (1, 0, 1, 0))), undo)
    elif what == "half":                            # mode() reads the first latent_channels: hand it the other half
        qc, lc = ref.quant_conv, ref.cfg.latent_channels
        _patch(qc, lambda x: F.conv2d(x, qc.weight, qc.bias).roll(lc, dims=1), undo)
    elif what == "pos":
        pe = ref.vision_model.embeddings.position_embedding
        _patch(pe, lambda ids: F.embedding(ids, pe.weight).roll(1, dims=-2), undo)
    elif what == "preln":
        _patch(ref.vision_model.pre_layrnorm, lambda x: x, undo)
    elif what == "pooled":                          # pooled = post_layernorm(last_hidden_state[:, 1])
        enc, orig = ref.vision_model.encoder, ref.vision_model.encoder.forward

        def shifted(*a, **kw):
            out = orig(*a, **kw)
            out.last_hidden_state = out.last_hidden_state.roll(-1, dims=1)
            return out
        _patch(enc, shifted, undo)
    else:
        raise KeyError(what)


def _apply_block(mut: Mutant, m, undo):
    if mut.family == "vae_attn":
        _patch(m, functools.partial(_vae_attention, m, mut.what), undo)
    elif mut.family == "dec_res":
        _patch(m, functools.partial(_res_block, m, mut.what), undo)
    elif mut.family == "clip_attn":
        _patch(m.self_attn, functools.partial(_clip_attention, m.self_attn, mut.what), undo)
    else:                                           # "act": the other of gelu / quick_gelu
        mlp = m.mlp
        quick = mlp.config.hidden_act == "quick_gelu"
        _patch(mlp, lambda x: mlp.fc2(F.gelu(mlp.fc1(x)) if quick else mlp.fc1(x) * torch.sigmoid(1.702 * mlp.fc1(x))), undo)


def _targets(mut: Mutant, ref):
    """(name, module) of the captured blocks a block-level mutant changes."""
    for name, m in ref.named_modules():
        if mut.family == "vae_attn" and isinstance(m, V._Attention):
            yield name, m
        elif mut.family == "dec_res" and isinstance(m, V.SpatioTemporalResBlock):
            if mut.what != "noshortcut" or m.spatial_res_block.conv_shortcut is not None:
                yield name, m
        elif (mut.family == "clip_attn" or mut.what == "act") and type(m).__name__ == "CLIPEncoderLayer":
            yield name, m


@contextlib.contextmanager
def mutate(oracle, mut: Mutant, block: str | None = None):
    """Apply ``mut`` everywhere it applies, or (block-level mutants) to the one block named by the oracle's module path.
    Yields the names of the blocks changed (model-level mutants: ``["*"]``)."""
    undo, hit = [], []
    try:
        if mut.in_block:
            for name, m in _targets(mut, oracle):
                if block is None or block == name:
                    _apply_block(mut, m, undo)
                    hit.append(name)
        else:
            assert block is None, f"{mut.name} does not sit inside a block"
            _apply_model(mut, oracle, undo)
            hit.append("*")
        yield hit
    finally:
        for u in reversed(undo):
            u()


# ------------------------------------------------------------------------------------------------ bounds and the table
def noise_and_bounds(ref, case: Case, x):
    """The fp32 oracle and its fp16-storage emulation on the same inputs -> (want, blocks, noise) with ``noise`` =
    {"final": e, "out": [per block], "branch": [per block], "emu": the emulation's final output}: the emulation's
    relative L2 error of each quantity.  The engine's bound for a quantity is FACTOR x its noise."""
    with capture_oracle(ref, keep_args=True) as blocks:
        want = run_oracle(ref, case, x)
    with fp16_storage(ref), capture_oracle(ref) as emu:
        got = run_oracle(ref, case, x)
    if case.model != "clip" and case.kind != "latents":
        got = got.half().float()                    # these engine calls return fp16
    noise = {"final": rel_l2(got, want), "out": [rel_l2(e.y, o.y) for e, o in zip(emu, blocks)],
             "branch": [rel_l2(e.branch, o.branch) for e, o in zip(emu, blocks)], "emu": got}
    return want, blocks, noise


def peak_statistics(ref, case: Case, x):
    """Per self-attention module, in call order: (name, logit standard deviation, mean largest probability of a row,
    1 / keys)."""
    stats, hooks = [], []

    def record(name, q, k, scale):
        logits = q @ k.transpose(-1, -2) * scale
        stats.append((name, float(logits.std()), float(logits.softmax(-1).amax(-1).mean()), 1.0 / logits.shape[-1]))

    for name, m in ref.named_modules():
        if isinstance(m, V._Attention):
            def hook(att, args, out, name=name):
                n, c, h, w = args[0].shape
                t = att.group_norm(args[0].reshape(n, c, h * w)).transpose(1, 2)
                record(name, att.to_q(t), att.to_k(t), 1.0 / math.sqrt(c))
            hooks.append(m.register_forward_hook(hook))
        elif type(m).__name__ == "CLIPAttention":
            def hook(att, args, kwargs, out, name=name):
                t = kwargs["hidden_states"] if "hidden_states" in kwargs else args[0]
                q, k = [p(t).view(*t.shape[:2], att.num_heads, att.head_dim).transpose(1, 2) for p in (att.q_proj, att.k_proj)]
                record(name, q, k, att.scale)
            hooks.append(m.register_forward_hook(hook, with_kwargs=True))
    try:
        run_oracle(ref, case, x)
    finally:
        for h in hooks:
            h.remove()
    return stats


def run_block_alone(ref, blk: Block):
    mod = dict(ref.named_modules())[blk.name]
    with torch.no_grad():
        return _rows(mod(*blk.args))


@functools.lru_cache(maxsize=None)
def sensitivity(case_name):
    """Everything the CPU test asserts for one case: the emulation's noise, and what every mutant moves -- applied
    everywhere: the final output; applied to one block: that block's branch, evaluated by running the block alone on its
    input of the clean forward (the blocks in front of it are unchanged, so this IS the block's branch in the mutated
    network).  ``decode_latents`` runs the decoder once per chunk: its blocks appear once per call."""
    case = CASES[case_name]
    ref = peaked_oracle(case.oracle_key)
    x = case_inputs(case)
    want, blocks, noise = noise_and_bounds(ref, case, x)
    out = {"case": case_name, "finite": bool(torch.isfinite(want).all() and all(torch.isfinite(b.y).all() for b in blocks)),
           "noise": noise, "blocks": [(b.name, b.kind) for b in blocks], "all": {}, "one": {}, "skipped": [],
           "peaks": peak_statistics(ref, case, x)}
    for mut in MUTANTS:
        if not applies(mut, case):
            if case.model in engines(mut):
                out["skipped"].append(mut.name)     # a mutant of this engine that this case cannot show
            continue
        with mutate(ref, mut):
            out["all"][mut.name] = rel_l2(run_oracle(ref, case, x), want)
        if not mut.in_block:
            continue
        per = out["one"][mut.name] = {}
        for i, blk in enumerate(blocks):
            with mutate(ref, mut, block=blk.name) as hit:
                if hit:
                    y = run_block_alone(ref, blk)
                    per[i] = rel_l2(Block("", blk.kind, blk.x, y).branch, blk.branch)
    return out


def format_table(s) -> str:
    n, blocks = s["noise"], s["blocks"]
    t_final = FACTOR * n["final"]
    lines = [f"case {s['case']}: fp16-storage noise of the final output {n['final']:.2e}, engine bound T = {t_final:.2e}"]
    for name, std, pmax, flat in s["peaks"]:
        lines.append(f"  {name}: logit standard deviation {std:.2f}, mean largest probability of a row {pmax:.3f} "
                     f"(a plain average: {flat:.4f})")
    lines += ["", "  mutant applied EVERYWHERE: displacement of the final output (rel-L2), and as a multiple of T"]
    for name, d in s["all"].items():
        lines.append(f"    {name:<50s} {d:9.2e}  {d / t_final:7.1f} x T")
    for name in s["skipped"]:
        lines.append(f"    {name:<50s} cannot show in this case")
    names = [m for m in s["one"] if s["one"][m]]
    lines += ["", "  mutant applied to ONE block: displacement of that block's branch (output - input; a width-changing resnet's:",
              f"  output) as a multiple of the block's own T = {FACTOR:g} x noise of its branch ('-': not in this block); columns:"]
    lines += [f"    {chr(97 + j)} = {m}" for j, m in enumerate(names)]
    lines.append(f"    {'block':<36s} {'noise out':>9s} {'branch':>9s}  " + " ".join(f"{chr(97 + j):>6s}" for j in range(len(names))))
    for i, (bname, kind) in enumerate(blocks):
        tb = FACTOR * n["branch"][i]
        cells = " ".join(f"{s['one'][m][i] / tb:6.1f}" if i in s["one"][m] else f"{'-':>6s}" for m in names)
        lines.append(f"    {i:2d} {bname:<33s} {n['out'][i]:9.2e} {n['branch'][i]:9.2e}  {cells}")
    return "\n".join(lines)


def plain_weights_record():
    """The state before this module, at the real widths and the shapes of the existing whole-model tests: under plain
    random weights the attention may be replaced by a mean of V, or run with a doubled scale, and the compared output
    moves by less than the 2e-2 (VAE decoder) / 1e-2 (CLIP) those tests allow."""
    from vdpp_amd.models.vae_hip import VAEDecoderConfig, random_state_dict
    out = {}
    case = Case("decoder, SVD widths, 2 x 24 x 32 latent", "decoder", "decode", 1, 2, 24, 32)
    ref = V.TemporalDecoderRef(V.VAEDecoderConfig.svd()).eval()
    ref.load_state_dict({k: v.float() for k, v in random_state_dict(VAEDecoderConfig.svd(), seed=2).items()}, strict=True)
    x = (torch.randn(2, 4, 24, 32, generator=torch.Generator().manual_seed(21)) * 4.0).half()
    clip = Case("clip, ViT-H/14 widths, 257 tokens, 4 layers", "clip", "vith4", 1)
    cref = plain_clip_model(clip_config("vith4"))
    px = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(9)).half()
    for c, r, inp, names in ((case, ref, x, ("vae attention: softmax -> mean of V", "vae attention: logits x2")),
                             (clip, cref, px, ("clip: softmax -> mean of V", "clip: scale x2"))):
        want = run_oracle(r, c, inp)
        rec = out[c.name] = {"peaks": peak_statistics(r, c, inp)}
        with fp16_storage(r):
            rec["fp16-storage noise"] = rel_l2(run_oracle(r, c, inp), want)
        for name in names:
            with mutate(r, by_name(name)):
                rec[name] = rel_l2(run_oracle(r, c, inp), want)
    return out


def main():
    print("Sensitivity of the edge engines' parity tests under the peaked state dicts (tiny(64) VAE, seed 3; CLIP by the _pair")
    print(f"recipe): the fp32 oracles alone, on the CPU.  Engine bound T = {FACTOR:g} x fp16-storage noise of the same quantity;")
    print(f"a mutant must reach {MARGIN:g} x T.\n")
    for name in CASES:
        print(format_table(sensitivity(name)))
        print()
    print("plain random weights at the real widths (the existing whole-model tests allow 2e-2 for the VAE, 1e-2 for CLIP):")
    for cname, rec in plain_weights_record().items():
        print(f"  {cname}")
        for name, std, pmax, flat in rec.pop("peaks"):
            print(f"    {name}: logit standard deviation {std:.2f}, largest probability {pmax:.4f} (a plain average: {flat:.4f})")
        for name, d in rec.items():
            print(f"    {name:<50s} {d:9.2e}")


if __name__ == "__main__":
    main()
