"""What the HIP engines (``unet_hip.py``, ``vae_hip.py``, ``clip_hip.py``) share: the device check, packed layers, the
record in which an activation travels from the kernel that wrote it to the kernel that reads it, the per-stream scratch
pool, and the base class that launches contractions and norms for all of them (``_Engine``)."""

from __future__ import annotations

import os
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


class StreamScratch:
    """Every per-stream scratch buffer of an engine: one uint8 tensor per (raw handle of the current HIP stream, name).
    Forwards on different streams may overlap in time, and two names never share an allocation.  Names in use: ``"gn"``
    GroupNorm partials, ``"splitk"`` split-K slabs, ``"fp8"`` fp8 attention operands, ``"long"`` flag words of the
    long-row attention."""

    def __init__(self, device):
        self.device, self._bufs = device, {}

    def get(self, name: str, nbytes: int, floor: int = 0) -> torch.Tensor:
        """The buffer of ``name`` on the current stream, at least ``nbytes`` long: the tensor handed out before while it
        is large enough, else a new one of ``max(nbytes, floor)`` bytes."""
        key = (torch.cuda.current_stream(self.device).cuda_stream, name)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._bufs[key] = torch.empty(max(nbytes, floor), dtype=torch.uint8, device=self.device)
        return buf

    def clear(self) -> None:
        self._bufs = {}


class _Engine:
    """Base of the engine classes: the device, the scratch pool, and the one place where a ``_Dense`` contraction, a
    GroupNorm and a LayerNorm statistics pass are launched -- with it the two rules of the statistics hand-off
    (``_gn_part_ok``: may a contraction's epilogue leave column sums for the GroupNorm behind it; ``_ln_out_ok``: row
    statistics for the folded LayerNorm behind it).  ``_groupnorm`` needs ``self.cfg.norm_groups``."""

    # rows up to which csrc/gemm.hip takes the small-tile / split-K routes (csrc/gemm.hip::SPLITK_MAX_ROWS); _ln_out_ok reads
    # it, and an engine that hands out split-K workspaces states its own beside that rule
    SPLITK_MAX_ROWS = 6144

    def __init__(self, device):
        self.device = hip_device(device, type(self).__name__)
        self._scratch = StreamScratch(self.device)
        # a norm's statistics out of the producing contraction's epilogue where a frame is whole 256-row tiles
        # (VDPP_GN_EPILOGUE=0: always the statistics pass)
        self.gn_from_epilogue = os.environ.get("VDPP_GN_EPILOGUE", "1") != "0"
        # ... also for outputs that residuals are added to (the final tile is rebuilt in LDS and summed there); 0: only
        # the no-residual producers (sums straight from the accumulators)
        self.gn_epilogue_residual = os.environ.get("VDPP_GN_EPILOGUE_RES", "1") != "0"
        # LayerNorm row statistics from the producing contraction's epilogue also for rows of three / four column tiles
        # (1,280 channels at the 576-token level)
        self.ln_out_wide = os.environ.get("VDPP_LN_OUT_WIDE", "1") != "0"

    def _buf(self, rows, c):
        return torch.empty((rows, c), dtype=torch.float16, device=self.device)

    def _gn_part_ok(self, layer: _Dense, m: int, frame_rows: int, epilogue: dict, *, ln_next=None, w_groups=None) -> bool:
        """May this contraction's epilogue leave per-tile column sums for the GroupNorm that reads its output?  Whole
        256-row tiles per frame, 256- / 320-wide column tiles over unpadded plain outputs, and nothing else in the
        epilogue that owns the final tile."""
        return bool(frame_rows and self.gn_from_epilogue and m % 256 == 0 and layer.n == layer.n_true
                    and not layer.geglu and (layer.n % 320 == 0 or layer.n % 256 == 0) and frame_rows % 256 == 0
                    and layer.colsum is None and ln_next is None and "euler" not in epilogue and w_groups is None
                    and (self.gn_epilogue_residual
                         or (epilogue.get("res1") is None and epilogue.get("res2") is None)))

    def _ln_out_ok(self, layer: _Dense, m: int) -> bool:
        """Can this contraction's epilogue leave the next LayerNorm's row statistics?  A row = one or two column tiles at
        any row count; three or four (1,024 / 1,280 channels: the 576-token level) only where the large ping-pong tiles
        are what the contraction runs on anyway (more rows than the small-tile / split-K routes take)."""
        if layer.n != layer.n_true or layer.geglu:
            return False
        return layer.n_true in (256, 320, 512, 640) or (self.ln_out_wide and layer.n_true in (768, 960, 1024, 1280)
                                                        and m > self.SPLITK_MAX_ROWS)

    def _dense(self, layer: _Dense, a, m, *, conv=None, temporal=None, frame_rows=0, ln_next=None, ln_out=None, out=None,
               weight=None, w_groups=None, workspace=None, **epilogue) -> _Act:
        """One contraction on the plain tensor ``a``; returns its output with the statistics the epilogue left.
        ``frame_rows`` > 0: the output goes straight into a GroupNorm (no residual in between) whose instances are
        multiples of that many rows (a frame): where ``_gn_part_ok`` the epilogue leaves per-tile column sums in the
        returned record and ``_groupnorm`` folds them instead of reading the tensor again.
        ``ln_next``: the contraction that will consume this output through a folded LayerNorm.  Where one tile spans a
        whole output row (256 / 320 channels: level 0) the epilogue leaves that LayerNorm's (mean, rstd) in the returned
        record and _ln_stats takes them from there instead of reading the tensor again (512 / 640 channels, level 1: two
        tiles per row, their sums meet in a 16-byte-per-row scratch).  ``ln_out``: the caller has decided that already
        and the statistics go there (a chunk's rows of the whole tensor's statistics).
        ``weight``: another pack of the layer's weights.  ``w_groups`` = (w_f [instances][n][c] fp16, bias_f
        [instances][n] fp32, rows per instance): a GroupNorm folded into this linear layer (ops.groupnorm_fold_linear) --
        every instance's rows meet their own scaled weights.  ``workspace``: split-K scratch for the few-row levels."""
        kw = epilogue
        weight, bias = layer.w if weight is None else weight, layer.bias
        if w_groups is not None:
            weight, bias = w_groups[0], None
            kw.update(bias2=w_groups[1], bias2_rows=w_groups[2], w_group_rows=w_groups[2],
                      w_group_stride=w_groups[0].shape[1] * w_groups[0].shape[2])
        gn_part = None
        if self._gn_part_ok(layer, m, frame_rows, kw, ln_next=ln_next, w_groups=w_groups):
            gn_part = torch.empty((m // 256, 2, layer.n, 2), dtype=torch.float32, device=self.device)
            kw.update(gn_part=gn_part)
        st = ln_out
        if st is None and ln_next is not None and self._ln_out_ok(layer, m) and "euler" not in kw:
            st = torch.empty((m, 2), dtype=torch.float32, device=self.device)
        if st is not None:
            kw.update(ln_out=st, ln_out_eps=ln_next.ln_eps)
            tiles = layer.n_true // (320 if layer.n_true % 320 == 0 else 256)
            workspace = torch.empty((m, 2 * tiles), dtype=torch.float32, device=self.device) if tiles > 1 else None
        if out is None:
            out = self._buf(m, layer.n_true)
        elif out.shape != (m, layer.n_true):
            raise RuntimeError(f"destination {tuple(out.shape)} does not match the contraction's output ({m}, {layer.n_true})")
        # operands may be column slices of wider row-major buffers (the halves of a concatenation buffer): row pitches
        # come from the tensors
        for key, ld in (("res1", "ldr1"), ("res2", "ldr2"), ("a2", "lda2")):
            if kw.get(key) is not None:
                kw.setdefault(ld, kw[key].stride(0))
        n_store = layer.n_true if (layer.n_true != (layer.n // 2 if layer.geglu else layer.n)) else 0
        if layer.colsum is not None and "ln_stats" not in kw:
            raise RuntimeError("this contraction carries a folded LayerNorm: pass ln_stats")
        ops.gemm(a, weight, out, m=m, n=layer.n, cin=layer.cin, mode=layer.mode, conv=conv, temporal=temporal,
                 bias=bias, geglu=layer.geglu, n_store=n_store, ldd=out.stride(0), lda=a.stride(0),
                 ln_colsum=layer.colsum, workspace=workspace, **kw)
        return _Act(out, gn_part=gn_part, ln_stats=st, ln_eps=ln_next.ln_eps if st is not None else None)

    def _ln_stats(self, layer: _Dense, x: _Act):
        """(mean, rstd) per row of x for the LayerNorm folded into ``layer``: left by x's producer, or a pass over x."""
        if x.ln_stats is not None and x.ln_eps == layer.ln_eps:
            return x.ln_stats
        return self._ln_pass(layer, x.t)

    def _ln_pass(self, layer: _Dense, x, **kw):
        st = torch.empty((x.shape[0], 2), dtype=torch.float32, device=self.device)
        ops.ln_stats(x, st, rows=x.shape[0], c=x.shape[1], eps=layer.ln_eps, **kw)
        return st

    def _groupnorm(self, norm: _Norm, a: _Act, instances, rows, silu, ws=None):
        """GroupNorm of ``a`` -> plain tensor.  Where a's producer left its column sums (for a concatenation buffer: both
        producers, an up block's first norm) and an instance is whole 256-row tiles, they replace the statistics pass;
        the pass takes its partial-sum scratch from ``ws`` or from the pool."""
        x, c, groups = a.t, a.t.shape[1], self.cfg.norm_groups
        y = self._buf(x.shape[0], c)
        if a.gn_part is not None and rows % 256 == 0:
            stats = torch.empty((instances, groups, 2), dtype=torch.float32, device=self.device)
            cat = dict(part_b=a.gn_part_b, c_a=a.c_a) if a.gn_part_b is not None else {}
            ops.groupnorm_tile_sums(x, a.gn_part, norm.g, norm.b, y, instances=instances, rows=rows, c=c, groups=groups,
                                    eps=norm.eps, silu=silu, stats=stats, ldx=x.stride(0), **cat)
            return y
        if ws is None:
            ws = self._scratch.get("gn", ops.groupnorm_ws_bytes(instances, rows, c, groups), floor=1 << 20)
        ops.groupnorm(x, norm.g, norm.b, y, instances=instances, rows=rows, c=c, groups=groups,
                      eps=norm.eps, silu=silu, ws=ws, ldx=x.stride(0))
        return y
