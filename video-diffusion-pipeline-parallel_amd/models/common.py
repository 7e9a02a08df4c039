"""What the HIP engines (``unet_hip.py``, ``vae_hip.py``, ``clip_hip.py``) share: the device check, packed layers, and
the record in which an activation travels from the kernel that wrote it to the kernel that reads it."""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..hip import ops
from . import weights as W


def hip_device(device, engine: str) -> torch.device:
    """The device an engine runs on; there is no CPU path, and a missing extension fails here."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{engine} runs on an MI355X HIP device only (no CPU fallback)")
    ops.load()
    return dev


def _f32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


@dataclass
class _Act:
    """An fp16 row tensor (possibly a column slice of a wider buffer) with the norm statistics its producer's epilogue
    left.  Statistics exist only on the record a producer returned: whoever slices rows, takes a view or writes the
    tensor in place goes on with a bare ``_Act(t)`` (or the plain tensor), and the consumer runs its statistics pass."""
    t: torch.Tensor
    gn_part: torch.Tensor = None    # per-tile column sums (sp_gemm_desc.gn_part) for the GroupNorm that follows ...
    gn_part_b: torch.Tensor = None  # ... of a concatenation buffer: gn_part covers the left c_a columns, this the rest
    c_a: int = 0
    ln_stats: torch.Tensor = None   # fp32 [rows][2] (mean, rstd) for the folded LayerNorm that follows (sp_gemm_desc.ln_out)
    ln_eps: float = None            # ... computed for this eps


class _Dense:
    """One contraction: packed fp16 weight ``[N][K]`` + fp32 bias, and how its A operand is gathered."""

    def __init__(self, w16, bias32, *, cin, mode=ops.A_LINEAR, n_true=None, geglu=False, colsum=None, ln_eps=None):
        self.w, self.bias, self.cin, self.mode = w16, bias32, cin, mode
        self.n = w16.shape[0]
        self.n_true = n_true if n_true is not None else (self.n // 2 if geglu else self.n)
        self.geglu = geglu
        self.colsum, self.ln_eps = colsum, ln_eps          # set when a LayerNorm is folded into this contraction

    @staticmethod
    def fold_layernorm(w, b, norm_w, norm_b, dev, *, eps, geglu=False):
        """``LN(x) @ W^T + b`` as a contraction on the un-normalised x: ``rstd*(x @ (W*gamma)^T - mean*colsum) + (W @ beta
        + b)`` with ``colsum[n] = sum_k (W*gamma)[n][k]`` taken over the fp16 values the kernel multiplies with."""
        w32, g32, be32 = w.to(dev).float(), norm_w.to(dev).float(), norm_b.to(dev).float()
        bias = w32 @ be32 + (b.to(dev).float() if b is not None else 0.0)
        wg = (w32 * g32[None, :])
        if geglu:
            wg, bias = W.interleave_geglu(wg, bias)
        wg16 = wg.to(torch.float16).contiguous()
        return _Dense(wg16, bias.float().contiguous(), cin=wg16.shape[1], geglu=geglu,
                      colsum=wg16.float().sum(dim=1).contiguous(), ln_eps=eps)

    @staticmethod
    def linear(sd, p, dev, bias=True):
        w = W.pack_linear(sd[p + ".weight"]).to(dev)
        return _Dense(w, _f32(sd[p + ".bias"], dev) if bias else None, cin=w.shape[1])

    @staticmethod
    def conv3x3(sd, p, dev):
        w = sd[p + ".weight"]
        cout, cin = w.shape[:2]
        npad, cpad = W.round_up(cout, 64), W.round_up(cin, 64)
        b = torch.zeros(npad, dtype=torch.float32, device=dev)
        b[:cout] = sd[p + ".bias"].to(dev).float()
        return _Dense(W.pack_conv3x3(w.to(dev), cpad, npad), b, cin=cpad, mode=ops.A_CONV3X3, n_true=cout)

    @staticmethod
    def tconv(sd, p, dev):
        w = sd[p + ".weight"]
        return _Dense(W.pack_tconv3(w.to(dev)), _f32(sd[p + ".bias"], dev), cin=w.shape[1], mode=ops.A_TEMPORAL3)

    @staticmethod
    def geglu_proj(sd, p, dev):
        wi, bi = W.interleave_geglu(sd[p + ".weight"].to(dev), sd[p + ".bias"].to(dev))
        return _Dense(wi, bi, cin=wi.shape[1], geglu=True)


class _Norm:
    def __init__(self, sd, p, dev, eps):
        self.g, self.b, self.eps = _f32(sd[p + ".weight"], dev), _f32(sd[p + ".bias"], dev), eps
