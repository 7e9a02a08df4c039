"""Can the whole-UNet parity tests see attention?  Helpers for tests/test_unet_sensitivity_cpu.py and
tests/test_unet_peaked_gpu.py (plain module: no fixtures, no tests; ``python -m tests.unet_mutants`` prints the table
kept in profiles/unet_sensitivity.txt).

* ``peaked_state_dict``  ``random_state_dict`` with the self-attention Q/K (and V) projections scaled up, so that the
  softmax rows have a peak and a wrong softmax moves the output by far more than fp16 storage does.  Under the plain
  U(+-1/sqrt(fan_in)) weights the logits have a standard deviation of 0.3 and every softmax is an average: attention
  may be replaced by a mean of V in all 16 transformers and the UNet output moves by 1.5e-2.
* ``MUTANTS``  plausible engine bugs, applied to the ORACLE at run time (context manager ``mutate``; oracle/ is not
  edited): per family (spatial, temporal) softmax -> mean, scale x2, last key dropped, K/V heads rotated against Q;
  temporal only: the neighbouring pixel's sequence, the other video's K/V, the frame position embedding dropped / off by
  one / reversed; controls: AlphaBlender operands swapped, GEGLU halves swapped.  All blocks or one named block.
* ``fp16_storage``  the oracle with the output of every Linear / Conv / GroupNorm / LayerNorm rounded to fp16: the noise
  floor that a bound for the engine is derived from (``T = FACTOR x noise``, per quantity).
* ``capture_oracle`` / ``capture_engine``  input and output of every resnet and transformer block as [rows][C], in call
  order (down, mid, up), from forward hooks on the oracle and from wrappers around ``SVDUNetHIP._run_resblock`` /
  ``_run_transformer`` of the instance under test.
"""
from __future__ import annotations

import contextlib
import functools
import math
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import svd_unet_ref as R

FACTOR = 3.0          # engine bound = FACTOR x the fp16-storage emulation's error of the same quantity
MARGIN = 2.0          # a mutant must move that quantity by MARGIN x the bound
SEED = 3
# (videos, frames, h, w): the shapes of the GPU tests and of the CPU sensitivity table
CASES = {"1x14x8x16": (1, 14, 8, 16), "1x25x8x8": (1, 25, 8, 8), "2x3x16x24": (2, 3, 16, 24)}
TIMESTEP = 1.63777


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ weights, inputs
def peaked_state_dict(cfg, seed, qk_gain=3.0, v_gain=2.0, out_gain=0.5, dtype=torch.float16):
    """``random_state_dict`` with every self-attention's ``to_q`` / ``to_k`` weight x ``qk_gain`` (logits x qk_gain^2:
    standard deviation 0.3 -> 3), ``to_v`` x ``v_gain`` and ``to_out.0`` x ``out_gain``, rounded to ``dtype`` afterwards.
    The gains were tuned on the CPU against the conditions of tests/test_unet_sensitivity_cpu.py (figures at 14 frames,
    8 x 16): with ``out_gain`` 1 the attention branches are twice as large, fp16 storage alone moves the final output by
    3.2e-3 and the deepest blocks by 5e-3, and a frame index off by one in ONE block then moves its branch by only 1.1 x
    the engine's bound there; at 0.5 the noise is 1.2e-3 / 2.0e-3 and the weakest single-block mutant stands at 3.3 x.
    ``v_gain`` 3 (noise 1.1e-2) or ``out_gain`` 2 (2.9e-2) are on the way to chaos; qk 4 with v 2 is there (0.10)."""
    from vdpp_amd.models.unet_spec import random_state_dict
    sd = random_state_dict(cfg, seed=seed, dtype=torch.float32)
    gains = {".attn1.to_q.weight": qk_gain, ".attn1.to_k.weight": qk_gain, ".attn1.to_v.weight": v_gain,
             ".attn1.to_out.0.weight": out_gain}
    hit = 0
    for name in sd:
        for tail, gain in gains.items():
            if name.endswith(tail):
                sd[name] = sd[name] * gain
                hit += 1
    assert hit == 4 * 32, f"{hit} self-attention weights scaled, expected 4 x 32"     # 16 transformers x (spatial, temporal)
    return {k: v.to(dtype) for k, v in sd.items()}


def configs(c=64):
    from vdpp_amd.models.unet_spec import UNetConfig
    return UNetConfig.tiny(c), R.SVDUNetConfig.tiny(c)


def build_oracle(sd, c=64):
    ref = R.SVDUNetRef(R.SVDUNetConfig.tiny(c)).eval()
    ref.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return ref


def case_inputs(cfg, case):
    """fp16-rounded inputs of a case: sample (B,F,8,H,W), ctx (B,1,cross), ids (B,3).  Two videos differ in content, in
    scale and in conditioning."""
    b, frames, h, w = CASES[case]
    g = torch.Generator().manual_seed(11 + frames)
    sample = torch.randn(b, frames, 8, h, w, generator=g)
    if b > 1:
        sample[1] *= 1.7
    ctx = torch.randn(b, 1, cfg.cross_attention_dim, generator=g)
    ids = torch.tensor([[5.0, 127.0, 0.02]]).repeat(b, 1)
    return sample.half(), ctx.half(), ids.half()


def run_oracle(ref, sample, ctx, ids, t=TIMESTEP):
    with torch.no_grad():
        return ref(sample.float(), t, ctx.float(), ids.float())[0]


# ------------------------------------------------------------------------------------------------ fp16 storage
_STORED = (nn.Linear, nn.Conv2d, nn.Conv3d, nn.GroupNorm, nn.LayerNorm)


@contextlib.contextmanager
def fp16_storage(oracle):
    """The oracle with fp16 STORAGE: the result of every Linear, Conv, GroupNorm and LayerNorm is rounded to fp16 (what
    an engine that keeps its activations in fp16 between kernels does at the least); arithmetic stays fp32."""
    hooks = [m.register_forward_hook(lambda mod, args, out: out.half().float())
             for m in oracle.modules() if isinstance(m, _STORED)]
    try:
        yield oracle
    finally:
        for h in hooks:
            h.remove()


# ------------------------------------------------------------------------------------------------ block capture
@dataclass
class Block:
    name: str             # the oracle's module path ("down_blocks.0.attentions.1"); engine side: "" (matched by position)
    kind: str             # "res" | "xf"
    x: torch.Tensor       # input  [rows][Cin]  (an up resnet's: running tensor and skip side by side)
    y: torch.Tensor       # output [rows][C]
    args: tuple = None    # oracle side, on request: the module's own arguments (to run the block alone)

    @property
    def branch(self):     # what the block adds to its input (transformers: Cin == C)
        return self.y.float() - self.x.float()


def _rows(t):             # (B*F, C, H, W) -> [rows][C], rows in (video, frame, y, x) order as the engine keeps them
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@contextlib.contextmanager
def capture_oracle(oracle, keep_args=False):
    rec, hooks = [], []
    for name, m in oracle.named_modules():
        kind = "res" if isinstance(m, R.SpatioTemporalResBlock) else "xf" if isinstance(m, R.TransformerSpatioTemporalModel) else None
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
    """Wraps ``_run_resblock`` / ``_run_transformer`` of this SVDUNetHIP instance.  Input and output are cloned at once:
    the views live in recycled or concatenation buffers, and a clone on the same stream is ordered behind the producer."""
    rec = []

    def wrap(kind, orig):
        @functools.wraps(orig)
        def run(r, p, x, *a, **kw):
            xin = x.t.clone()
            y = orig(r, p, x, *a, **kw)
            rec.append(Block("", kind, xin, y.t.clone()))
            return y
        return run

    hip._run_resblock = wrap("res", hip._run_resblock)
    hip._run_transformer = wrap("xf", hip._run_transformer)
    try:
        yield rec
    finally:
        del hip._run_resblock, hip._run_transformer


def assert_same_blocks(engine, oracle):
    assert [b.kind for b in engine] == [b.kind for b in oracle], "engine and oracle ran different block sequences"
    for e, o in zip(engine, oracle):
        assert e.x.shape == o.x.shape and e.y.shape == o.y.shape, f"{o.name}: {tuple(e.x.shape)} -> {tuple(e.y.shape)} " \
            f"against the oracle's {tuple(o.x.shape)} -> {tuple(o.y.shape)}"


# ------------------------------------------------------------------------------------------------ mutants
@dataclass(frozen=True)
class Mutant:
    name: str
    family: str           # "spatial" | "temporal" | "pos" | "control"
    what: str             # the attention / embedding / control variant, see _attention and _apply
    drop_key: bool = False


MUTANTS = (
    Mutant("spatial softmax -> mean of V", "spatial", "mean"),
    Mutant("spatial scale x2", "spatial", "scale2"),
    Mutant("spatial K/V heads rotated by one", "spatial", "heads"),
    Mutant("spatial last key dropped", "spatial", "dropkey", drop_key=True),
    Mutant("temporal softmax -> mean of V", "temporal", "mean"),
    Mutant("temporal scale x2", "temporal", "scale2"),
    Mutant("temporal K/V heads rotated by one", "temporal", "heads"),
    Mutant("temporal last frame's key dropped", "temporal", "dropkey", drop_key=True),
    Mutant("temporal sequence of the neighbouring pixel", "temporal", "pixel"),
    Mutant("temporal K/V of the other video", "temporal", "video"),
    Mutant("time_pos_embed dropped", "pos", "drop"),
    Mutant("time_pos_embed frame index off by one", "pos", "plus1"),
    Mutant("time_pos_embed frame order reversed", "pos", "reverse"),
    Mutant("control: AlphaBlender operands swapped", "control", "blender"),
    Mutant("control: GEGLU halves swapped", "control", "geglu"),
)


def by_name(name) -> Mutant:
    return next(m for m in MUTANTS if m.name == name)


def applies(mut: Mutant, block: nn.Module, videos: int) -> bool:
    """Whether the mutant changes anything in this block: head rotation needs two heads (level 0 of the tiny
    configuration has one), the other video's K/V two videos, everything but the blender control a transformer."""
    xf = isinstance(block, R.TransformerSpatioTemporalModel)
    if mut.what == "blender":
        return True
    if not xf:
        return False
    if mut.what == "heads":
        return block.transformer_blocks[0].attn1.heads > 1
    if mut.what == "video":
        return videos == 2
    return True


def is_identity(mut: Mutant, tokens: int) -> bool:
    """At one token per frame (the 8 x 8 latents' innermost level) a spatial softmax is 1 whatever the scale, and there
    is no neighbouring pixel: such a mutant changes nothing there and cannot be asked to show."""
    return tokens == 1 and ((mut.family == "spatial" and mut.what in ("mean", "scale2", "dropkey")) or mut.what == "pixel")


def _attention(att, what, info, x, context=None):
    """``oracle.svd_unet_ref.Attention.forward`` with one thing wrong.  ``info``: the enclosing transformer's batch size
    and frame count (temporal sequences arrive as (B*HW, F, C))."""
    if what == "pixel":          # every sequence is read one pixel further along (within its video)
        x = x.reshape(info["b"], -1, *x.shape[1:]).roll(-1, dims=1).reshape(x.shape)
    ctx = x if context is None else context
    if what == "video":
        ctx = x.reshape(info["b"], -1, *x.shape[1:]).flip(0).reshape(x.shape)
    b, n, _ = x.shape
    q = att.to_q(x).view(b, n, att.heads, -1).transpose(1, 2)
    k = att.to_k(ctx).view(b, ctx.shape[1], att.heads, -1).transpose(1, 2)
    v = att.to_v(ctx).view(b, ctx.shape[1], att.heads, -1).transpose(1, 2)
    if what == "heads":
        k, v = k.roll(1, dims=1), v.roll(1, dims=1)
    if what == "dropkey" and k.shape[2] > 1:
        k, v = k[:, :, :-1], v[:, :, :-1]
    if what == "mean":
        o = v.mean(dim=2, keepdim=True).expand_as(q)
    else:
        o = F.scaled_dot_product_attention(q, k, v, scale=(2.0 if what == "scale2" else 1.0) / math.sqrt(q.shape[-1]))
    return att.to_out[0](o.transpose(1, 2).reshape(b, n, -1))


def _apply(mut: Mutant, block: nn.Module, undo: list):
    """Patch ``forward`` of the instances concerned (instance attributes: removed again by ``undo``)."""
    info = {}

    def patch(mod, fn):
        mod.forward = fn
        undo.append(lambda: mod.__delattr__("forward"))

    if mut.what == "blender":
        mixer, orig = block.time_mixer, block.time_mixer.forward
        patch(mixer, lambda a, b: orig(b, a))
        return
    if mut.what == "geglu":
        for g in [m for m in block.modules() if isinstance(m, R.GEGLU)]:
            def swapped(x, g=g):
                h, gate = g.proj(x).chunk(2, dim=-1)
                return gate * F.gelu(h)
            patch(g, swapped)
        return
    pre = block.register_forward_pre_hook(lambda mod, args: info.update(b=args[0].shape[0] // args[2], nf=args[2]))
    undo.append(pre.remove)
    if mut.family == "pos":
        tpe, orig = block.time_pos_embed, block.time_pos_embed.forward

        def embed(s):
            f = torch.arange(info["nf"], device=s.device)
            f = {"plus1": f + 1, "reverse": info["nf"] - 1 - f, "drop": f}[mut.what].repeat(info["b"])
            e = orig(R.sinusoid(f, block.channels).to(s.dtype))
            return torch.zeros_like(e) if mut.what == "drop" else e
        patch(tpe, embed)
        return
    blk = block.transformer_blocks[0] if mut.family == "spatial" else block.temporal_transformer_blocks[0]
    patch(blk.attn1, functools.partial(_attention, blk.attn1, mut.what, info))


@contextlib.contextmanager
def mutate(oracle, mut: Mutant, videos: int, block: str | None = None):
    """Apply ``mut`` to every block it applies to, or to the one block named (the oracle's module path).  Yields the
    names of the blocks changed."""
    undo, hit = [], []
    try:
        for name, m in oracle.named_modules():
            if not isinstance(m, (R.SpatioTemporalResBlock, R.TransformerSpatioTemporalModel)):
                continue
            if (block is None or block == name) and applies(mut, m, videos):
                _apply(mut, m, undo)
                hit.append(name)
        yield hit
    finally:
        for u in reversed(undo):
            u()


# ------------------------------------------------------------------------------------------------ bounds and the table
def noise_and_bounds(ref, sample, ctx, ids, t=TIMESTEP):
    """The fp32 oracle and its fp16-storage emulation on the same inputs -> (want, blocks, noise) with ``noise`` =
    {"final": e, "out": [per block], "branch": [per block; None for resnets], "emu": the emulation's final output}: the
    emulation's relative L2 error of each quantity.  The engine's bound for a quantity is FACTOR x its noise.  Nothing here comes from the engine."""
    with capture_oracle(ref, keep_args=True) as blocks:
        want = run_oracle(ref, sample, ctx, ids, t)
    with fp16_storage(ref), capture_oracle(ref) as emu:
        got = run_oracle(ref, sample, ctx, ids, t)
    noise = {"final": rel_l2(got, want), "out": [rel_l2(e.y, o.y) for e, o in zip(emu, blocks)],
             "branch": [rel_l2(e.branch, o.branch) if o.kind == "xf" else None for e, o in zip(emu, blocks)],
             "emu": got}
    return want, blocks, noise


def peak_statistics(ref, sample, ctx, ids):
    """How peaked the self-attention rows are: per family the standard deviation of the logits and the mean largest
    probability of a row, averaged over the 16 transformers (a plain average over n keys has 1 / n)."""
    stats, hooks = {"spatial": [], "temporal": []}, []
    for m in ref.modules():
        if isinstance(m, R.TransformerSpatioTemporalModel):
            for fam, att in (("spatial", m.transformer_blocks[0].attn1), ("temporal", m.temporal_transformer_blocks[0].attn1)):
                def hook(att, args, out, fam=fam):
                    x = args[0]
                    q = att.to_q(x).view(*x.shape[:2], att.heads, -1).transpose(1, 2)
                    k = att.to_k(x).view(*x.shape[:2], att.heads, -1).transpose(1, 2)
                    logits = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
                    if logits.shape[-1] > 1:
                        stats[fam].append((float(logits.std()), float(logits.softmax(-1).amax(-1).mean()), logits.shape[-1]))
                hooks.append(att.register_forward_hook(hook))
    try:
        run_oracle(ref, sample, ctx, ids)
    finally:
        for h in hooks:
            h.remove()
    return {fam: (sum(v[0] for v in vs) / len(vs), sum(v[1] for v in vs) / len(vs), sum(1.0 / v[2] for v in vs) / len(vs))
            for fam, vs in stats.items()}


@functools.lru_cache(maxsize=None)
def sensitivity(case, qk_gain=3.0, v_gain=2.0, out_gain=0.5):
    """Everything the CPU test asserts for one case: noise of the emulation, and what every mutant moves -- applied to
    all blocks: the final output; applied to one transformer: that block's branch (output - input), evaluated by running
    the block alone on its input of the clean forward (the blocks in front of it are unchanged, so this IS the block's
    branch in the mutated network).  The controls are applied to all blocks only: a blender whose mix factor happens to
    be near 0 (alpha = 0.5) does not care about the order of its operands."""
    cfg, _ = configs()
    videos = CASES[case][0]
    ref = build_oracle(peaked_state_dict(cfg, SEED, qk_gain, v_gain, out_gain))
    sample, ctx, ids = case_inputs(cfg, case)
    want, blocks, noise = noise_and_bounds(ref, sample, ctx, ids)
    mods = dict(ref.named_modules())
    out = {"case": case, "finite": bool(torch.isfinite(want).all() and all(torch.isfinite(b.y).all() for b in blocks)),
           "noise": noise, "blocks": [(b.name, b.kind) for b in blocks], "all": {}, "one": {},
           "peaks": peak_statistics(ref, sample, ctx, ids)}
    for mut in MUTANTS:
        with mutate(ref, mut, videos) as hit:
            if not hit:
                continue
            out["all"][mut.name] = rel_l2(run_oracle(ref, sample, ctx, ids), want)
        if mut.family == "control":
            continue
        per = out["one"][mut.name] = {}
        for i, blk in enumerate(blocks):
            tokens = blk.args[0].shape[2] * blk.args[0].shape[3]
            with mutate(ref, mut, videos, block=blk.name) as hit:
                if not hit or is_identity(mut, tokens):
                    continue
                with torch.no_grad():
                    y = _rows(mods[blk.name](*blk.args))
            per[i] = rel_l2(y - blk.x, blk.branch)
    return out


def format_table(s) -> str:
    n, blocks = s["noise"], s["blocks"]
    t_final = FACTOR * n["final"]
    lines = [f"case {s['case']}: fp16-storage noise of the final output {n['final']:.2e}, engine bound T = {t_final:.2e}"]
    for fam, (std, pmax, flat) in s["peaks"].items():
        lines.append(f"  {fam} self-attention: logit standard deviation {std:.2f}, mean largest probability of a row {pmax:.3f} "
                     f"(a plain average: {flat:.3f})")
    lines += ["", "  mutant applied to ALL blocks: displacement of the final output (rel-L2), and as a multiple of T"]
    for name, d in s["all"].items():
        lines.append(f"    {name:<48s} {d:9.2e}  {d / t_final:7.1f} x T")
    names = [m for m in s["one"] if s["one"][m]]
    lines += ["", "  mutant applied to ONE transformer: displacement of that block's branch (output - input) as a multiple of the",
              "  block's own T = 3 x noise of its branch ('-': the mutant changes nothing in this block); columns:"]
    lines += [f"    {chr(97 + j)} = {m}" for j, m in enumerate(names)]
    lines.append(f"    {'block':<32s} {'noise out':>9s} {'branch':>9s}  " + " ".join(f"{chr(97 + j):>5s}" for j in range(len(names))))
    for i, (bname, kind) in enumerate(blocks):
        if kind == "res":
            lines.append(f"    {i:2d} {bname:<29s} {n['out'][i]:9.2e}")
            continue
        tb = FACTOR * n["branch"][i]
        cells = " ".join(f"{s['one'][m][i] / tb:5.1f}" if i in s["one"][m] else f"{'-':>5s}" for m in names)
        lines.append(f"    {i:2d} {bname:<29s} {n['out'][i]:9.2e} {n['branch'][i]:9.2e}  {cells}")
    return "\n".join(lines)


def plain_weights_record(case="1x14x8x16"):
    """The state before this module: under plain ``random_state_dict`` the all-block temporal-mean mutant moves the final
    output by less than the 2e-2 the whole-UNet tests allow."""
    from vdpp_amd.models.unet_spec import random_state_dict
    cfg, _ = configs()
    ref = build_oracle(random_state_dict(cfg, seed=SEED, dtype=torch.float16))
    sample, ctx, ids = case_inputs(cfg, case)
    want = run_oracle(ref, sample, ctx, ids)
    out = {"peaks": peak_statistics(ref, sample, ctx, ids)}
    for name in ("temporal softmax -> mean of V", "spatial softmax -> mean of V"):
        with mutate(ref, by_name(name), CASES[case][0]):
            out[name] = rel_l2(run_oracle(ref, sample, ctx, ids), want)
    return out


def main():
    print("UNet sensitivity under peaked_state_dict(tiny(64), seed=3, qk_gain=3, v_gain=2, out_gain=0.5): the fp32 oracle alone,")
    print(f"on the CPU.  Engine bound T = {FACTOR:g} x fp16-storage noise of the same quantity; a mutant must reach {MARGIN:g} x T.\n")
    for case in CASES:
        print(format_table(sensitivity(case)))
        print()
    rec = plain_weights_record()
    print("plain random_state_dict, case 1x14x8x16, all blocks (the existing whole-UNet tests allow 2e-2):")
    for fam, (std, pmax, flat) in rec.pop("peaks").items():
        print(f"  {fam} self-attention: logit standard deviation {std:.2f}, mean largest probability of a row {pmax:.3f} "
              f"(a plain average: {flat:.3f})")
    for name, d in rec.items():
        print(f"    {name:<48s} {d:9.2e}")


if __name__ == "__main__":
    main()
