#!/usr/bin/env python3
"""What the engines launch, as text that two versions of the Python package can be compared by.

Default (no GPU): whole forwards of the UNet, the VAE decoder / encoder and the CLIP encoder on CPU tensors with every
``hip.ops`` wrapper replaced by a recorder (``tests/launch_recorder.py``).  Per configuration the canonical log of every
recorded call -- its name and every argument after binding to the real wrapper's signature with defaults applied -- and
the SHA-256 of that log.  Scalars print by ``repr``; a tensor prints as dtype, shape, strides, buffer number (order of
first appearance of its storage in the run; every tensor stays alive) and byte offset inside the buffer.  The only
normalisation is ``DERIVED``: where a wrapper turns a ``None`` pitch into a value derived from another argument, the
derived value is printed.

    python tools/launch_identity.py [--out DIR] [--only NAME]     the logs (to DIR/NAME.log with --out) and the digests
    python tools/launch_identity.py --gpu                          SHA-256 of the outputs of fixed-seed runs on cuda:0

The tool loads the package of the tree it lies in: to compare two versions, copy it (and ``tests/launch_recorder.py``)
into a checkout of the other one and diff the outputs."""
import argparse
import hashlib
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import vdpp_amd  # noqa: E402,F401
from vdpp_amd.hip import ops  # noqa: E402
from vdpp_amd.models import clip_hip, unet_hip, vae_hip  # noqa: E402
from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict  # noqa: E402


def _nout(a):
    return a["n"] // 2 if a["geglu"] else a["n"]


# wrapper -> argument -> what ``None`` becomes inside the wrapper (the bound arguments go in)
DERIVED = {
    "gemm": dict(lda=lambda a: a["cin"], ldd=lambda a: a["n_store"] or _nout(a), ldr1=_nout, ldr2=_nout,
                 lda2=lambda a: a["a2"].stride(0) if a["a2"] is not None else None),
    "groupnorm": dict(ldx=lambda a: a["c"]),
    "groupnorm_fold_linear": dict(ldx=lambda a: a["c"]),
    "groupnorm_tile_sums": dict(ldx=lambda a: a["x"].stride(0)),
}


class Canon:
    """Canonical text of one run's launches."""

    def __init__(self, signatures):
        self.signatures, self.buffers = signatures, {}

    def value(self, v):
        if isinstance(v, torch.Tensor):
            base = v.untyped_storage().data_ptr()
            n = self.buffers.setdefault(base, len(self.buffers))
            return (f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}/{list(v.stride())}"
                    f"@buf{n}+{v.data_ptr() - base}")
        if isinstance(v, dict):
            return "{" + ", ".join(f"{k}: {self.value(v[k])}" for k in sorted(v)) + "}"
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(self.value(e) for e in v) + ")"
        return repr(v)

    def line(self, launch):
        bound = self.signatures[launch.name].bind(*launch.args, **launch.kw)
        bound.apply_defaults()
        a = bound.arguments
        for key, derive in DERIVED.get(launch.name, {}).items():
            if a[key] is None:
                a[key] = derive(a)
        return f"{launch.name}(" + ", ".join(f"{k}={self.value(v)}" for k, v in a.items()) + ")"


# ------------------------------------------------------------------------------------------------ configurations
def unet(c, shape, *, chunks=None, euler=False, env=None, per_video=False, **engine_kw):
    def run():
        with _environ(env):
            cfg = UNetConfig.tiny(c)
            hip = unet_hip.SVDUNetHIP(cfg, random_state_dict(cfg, seed=47, dtype=torch.float16), DEVICE, **engine_kw)
        if chunks:
            hip.FF_CHUNK_BYTES, hip.FF_CHUNK_ROUND = chunks
        b, f, _, h, w = shape
        gen = torch.Generator().manual_seed(11)
        sample = torch.randn(shape, generator=gen).half()
        ctx = torch.randn(b, 1, cfg.cross_attention_dim, generator=gen).half()
        ids = torch.tensor([[5.0 + i, 127.0 - 20 * i, 0.02] for i in range(b if per_video else 1)] * (1 if per_video else b))
        t = torch.tensor([0.6 - 0.25 * i for i in range(b)]) if per_video else 0.6

        def forward():
            if not euler:
                return hip(sample, t, ctx, ids, per_video=per_video)[0]
            dev = hip.device
            rows = torch.zeros((b * f * h * w, hip.cin_pad), dtype=torch.float16, device=dev)
            e = dict(latent=torch.zeros(b, 4, f, h, w, dtype=torch.float16, device=dev),
                     out=torch.zeros(b, 4, f, h, w, dtype=torch.float16, device=dev),
                     sigma=torch.zeros(1), sigma_next=torch.zeros(1))
            assert hip.forward_rows(rows, b=b, frames=f, h=h, w=w, t_value=torch.zeros(1, device=dev),
                                    ctx16=ctx.reshape(b, -1).to(dev), added_ids32=ids[0].to(dev), euler=e) is None
            return e["out"]
        return forward
    return run


def vae_decoder(call, *, env=None):
    def run():
        with _environ(env):
            cfg = vae_hip.VAEDecoderConfig.tiny(64)
            dec = vae_hip.TemporalDecoderHIP(cfg, vae_hip.random_state_dict(cfg, seed=1), DEVICE)
        gen = torch.Generator().manual_seed(12)
        return lambda: call(dec, lambda *shape: torch.randn(shape, generator=gen).half().to(dec.device))
    return run


def vae_encoder():
    cfg = vae_hip.VAEDecoderConfig.tiny(64)
    enc = vae_hip.ImageEncoderHIP(cfg, vae_hip.random_encoder_state_dict(cfg, seed=2), DEVICE)
    image = torch.rand((2, 3, 128, 128), generator=torch.Generator().manual_seed(13)).mul(2).sub(1).half().to(enc.device)
    return lambda: enc.encode_image_latents(image, 3)


def clip():
    spec = clip_hip.CLIPVisionSpec.tiny()
    enc = clip_hip.CLIPVisionHIP(spec, clip_hip.random_state_dict(spec, seed=3), DEVICE)
    pixels = torch.randn((2, 3, spec.image_size, spec.image_size), generator=torch.Generator().manual_seed(14))
    return lambda: enc(pixels.half().to(enc.device))


class _environ:
    """Environment variables for the time an engine is constructed (the switches are read there)."""

    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        return False


BASE = (2, 3, 8, 16, 16)
CONFIGS = [
    ("unet_c256_2x3x16x16", unet(256, BASE)),
    ("unet_c64_1x3x16x24", unet(64, (1, 3, 8, 16, 24))),
    ("unet_c256_1x2x32x32", unet(256, (1, 2, 8, 32, 32))),
    ("unet_c256_ff_chunks", unet(256, BASE, chunks=(1 << 18, 256))),
    ("unet_euler", unet(256, BASE, euler=True)),
    *[(f"unet_{s}_off", unet(256, BASE, env={s: "0"})) for s in
      ("VDPP_GN_EPILOGUE", "VDPP_GN_EPILOGUE_RES", "VDPP_FOLD_GN", "VDPP_FOLD_SHORTCUT", "VDPP_LN_OUT_WIDE")],
    ("unet_fp8_attention_1024_tokens", unet(256, (1, 2, 8, 32, 32), fp8_attention=True)),
    ("unet_long_rows_96x96", unet(64, (1, 1, 8, 96, 96))),
    ("unet_per_video", unet(256, BASE, per_video=True)),
    ("vae_decode_2x4x8x8", vae_decoder(lambda d, z: d.decode(z(2, 4, 8, 8), 2))),
    ("vae_decode_4x4x16x16", vae_decoder(lambda d, z: d.decode(z(4, 4, 16, 16), 2))),
    ("vae_decode_latents_chunk_straddles", vae_decoder(lambda d, z: d.decode_latents(z(2, 4, 3, 8, 8), 3, 2))),
    ("vae_decode_latents_uint8", vae_decoder(lambda d, z: d.decode_latents_uint8(z(2, 4, 3, 8, 8), 3, 2))),
    ("vae_decode_long_attn_from_0", vae_decoder(lambda d, z: d.decode(z(4, 4, 16, 16), 2),
                                                env={"VDPP_VAE_LONG_ATTN_FROM": "0"})),
    ("vae_decode_fp16_scores", vae_decoder(lambda d, z: d.decode(z(4, 4, 16, 16), 2), env={"VDPP_VAE_FP16_SCORES": "1"})),
    ("vae_encode_2x3x128x128", lambda: vae_encoder()),
    ("clip_tiny", lambda: clip()),
]
# --gpu: the outputs that are hashed
GPU_RUNS = ["unet_c256_2x3x16x16", "unet_c64_1x3x16x24", "vae_decode_4x4x16x16", "vae_encode_2x3x128x128", "clip_tiny"]
DEVICE = "cpu"


def main():
    global DEVICE
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="directory for one canonical log per configuration")
    ap.add_argument("--only", action="append", help="run this configuration only (may repeat)")
    ap.add_argument("--gpu", action="store_true", help="run on cuda:0 and print SHA-256 of the outputs")
    args = ap.parse_args()
    configs = [(n, f) for n, f in CONFIGS if (n in args.only if args.only else not args.gpu or n in GPU_RUNS)]
    if args.gpu:
        DEVICE = "cuda:0"
        torch.cuda.set_device(0)
        for name, make in configs:
            out = make()()
            torch.cuda.synchronize()
            data = out.cpu().contiguous()
            digest = hashlib.sha256(data.view(torch.uint8).numpy().tobytes()).hexdigest()
            print(f"{name}: output {str(out.dtype).replace('torch.', '')}{list(out.shape)} sha256 {digest}", flush=True)
        return
    signatures = {}
    from tests import launch_recorder
    for name in launch_recorder.wrapper_names():
        signatures[name] = inspect.signature(getattr(ops, name))
    launches = launch_recorder.install(setattr)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    for name, make in configs:
        forward = make()
        launches.clear()
        forward()
        canon = Canon(signatures)
        text = "".join(canon.line(l) + "\n" for l in launches)
        if args.out:
            with open(os.path.join(args.out, name + ".log"), "w") as fh:
                fh.write(text)
        else:
            sys.stdout.write(text)
        print(f"{name}: {len(launches)} calls, sha256 {hashlib.sha256(text.encode()).hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
