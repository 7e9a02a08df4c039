"""Tensor-level wrappers over the C ABI: raw ``data_ptr()`` + the current HIP stream go in,
kernels are enqueued, nothing is synchronised.  PyTorch only owns the memory."""

from __future__ import annotations

import ctypes

import torch

from . import GemmDesc, last_error, load

A_LINEAR, A_CONV3X3, A_TEMPORAL3 = 0, 1, 2
ZERO_PAGE_BYTES = 4096
_zero_pages: dict = {}


class HipKernelError(RuntimeError):
    pass


# Optional per-launch timing (bench.py roofline leg): when a list is installed here, the contraction
# and attention wrappers bracket their launch with events on the launching stream and append
# (kind, flops, start_event, end_event, algorithmic_bytes, tag) -- tag: the shape of a contraction, else None.
PROFILE = None


class _Timed:
    def __init__(self, kind, flops, nbytes=0.0, tag=None):
        self.kind, self.flops, self.nbytes, self.tag = kind, flops, nbytes, tag

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.append((self.kind, self.flops, self.e0, self.e1, self.nbytes, self.tag))
        return False


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise HipKernelError(f"{what} failed (rc={rc}): {last_error()}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def zero_page(device) -> torch.Tensor:
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(ZERO_PAGE_BYTES, dtype=torch.uint8, device=dev)
    return _zero_pages[key]


def _f16(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float16 or not t.is_cuda:
        raise TypeError(f"{name} must be a float16 tensor on a HIP device")
    if t.dim() >= 1 and t.stride(-1) != 1 and t.shape[-1] != 1:
        raise ValueError(f"{name} must be row-major (innermost stride 1); got strides {tuple(t.stride())}")
    return t


def _rows(t: torch.Tensor, name: str, ld: int) -> torch.Tensor:
    """2-D token matrix whose row pitch must equal the leading dimension handed to the kernel."""
    _f16(t, name)
    if t.dim() == 2 and t.shape[0] > 1 and t.stride(0) != ld:
        raise ValueError(f"{name}: row stride {t.stride(0)} does not match leading dimension {ld}")
    return t


def gemm(a, w, out, *, m, n, cin, mode=A_LINEAR, lda=None, conv=None, temporal=None, bias=None,
         bias2=None, bias2_rows=0, ldb2=0, res1=None, r1scale=1.0, res2=None, r2scale=1.0, oscale=1.0,
         geglu=False, n_store=0, ldd=None, ldr1=None, ldr2=None, ln_stats=None, ln_colsum=None, euler=None,
         workspace=None, ln_out=None, ln_out_eps=1e-5, w_group_rows=0, w_group_stride=0, gn_part=None, a2=None, cin2=0,
         lda2=None, up2x_phases=False):
    """``out[m][:] = epilogue(sum_taps A_tap @ W^T)``; see ``sp_gemm_desc`` in include/svdpipe.h.
    ``ln_stats`` / ``ln_colsum``: LayerNorm folded into the contraction (``a`` is the UN-normalised tensor).
    ``w_group_rows`` / ``w_group_stride``: ``w`` holds one weight matrix per group of that many output rows (a GroupNorm
    folded into this linear layer, ``groupnorm_fold_linear``).
    ``up2x_phases``: an upsampling convolution (``mode=A_CONV3X3``, ``conv[-1] == 1``) as four 2x2 phase convolutions;
    ``w`` is then the phase-major pack ``[4][n][4*cin]`` (``weights.pack_conv3x3_up2x``), bias only (``sp_conv_up2x_f16``)."""
    if up2x_phases:
        # the phase entry takes a bias and nothing else of the epilogue: every other keyword must be at its neutral value
        # (``workspace`` is scratch the call may leave unused; pitches and scales of absent operands mean nothing)
        refused = dict(temporal=(temporal, None), bias2=(bias2, None), res1=(res1, None), res2=(res2, None),
                       ln_stats=(ln_stats, None), ln_colsum=(ln_colsum, None), euler=(euler, None), ln_out=(ln_out, None),
                       a2=(a2, None), geglu=(bool(geglu), False), n_store=(n_store, 0), w_group_rows=(w_group_rows, 0),
                       oscale=(oscale, 1.0))
        extra = sorted(k for k, (v, neutral) in refused.items() if (v is not None if neutral is None else v != neutral))
        if extra:
            raise ValueError(f"gemm(up2x_phases=True) takes a bias only; got {', '.join(extra)}")
        return _conv_up2x(a, w, out, m=m, n=n, cin=cin, mode=mode, lda=lda, conv=conv, bias=bias, ldd=ldd, gn_part=gn_part)
    d = GemmDesc()
    d.lda = int(lda if lda is not None else cin)
    d.a, d.mode, d.cin = _rows(a, "a", d.lda).data_ptr(), mode, cin
    if mode == A_CONV3X3:
        d.n_img, d.hin, d.win, d.hout, d.wout, d.stride, d.upsample2x = conv
    if mode == A_TEMPORAL3:
        d.frames, d.hw = temporal
    d.w, d.m, d.n = _f16(w, "w").data_ptr(), m, n
    d.bias, d.bias2, d.bias2_rows, d.ldb2 = _ptr(bias), _ptr(bias2), bias2_rows, ldb2
    nout = n // 2 if geglu else n
    d.res1, d.ldr1, d.r1scale = _ptr(res1), int(ldr1 if ldr1 is not None else nout), r1scale
    d.res2, d.ldr2, d.r2scale = _ptr(res2), int(ldr2 if ldr2 is not None else nout), r2scale
    d.oscale, d.geglu, d.n_store = oscale, int(geglu), n_store
    d.ldd = int(ldd if ldd is not None else (n_store or nout))
    d.d = _rows(out, "out", d.ldd).data_ptr()
    d.zero_page = zero_page(a.device).data_ptr()
    d.ln_stats, d.ln_colsum = _ptr(ln_stats), _ptr(ln_colsum)
    if euler is not None:       # conv_out only: guidance mix + Euler update instead of storing eps rows (see svdpipe.h)
        d.euler_latent, d.euler_out = _f16(euler["latent"], "latent").data_ptr(), _f16(euler["out"], "out").data_ptr()
        d.euler_eps_uncond, d.euler_guidance = _ptr(euler.get("eps_uncond")), _ptr(euler.get("guidance"))
        d.euler_ld_eps = int(euler.get("ld_eps", 0))
        d.euler_guidance_ld = int(euler.get("ld_guidance", 0))     # guidance [B][ld] per video; 0: one [F] row for all
        d.euler_sigma, d.euler_sigma_next = float(euler["sigma"]), float(euler["sigma_next"])
        d.euler_frames, d.euler_hw = int(euler["frames"]), int(euler["hw"])
    if workspace is not None:      # fp32 scratch: split-K (few rows, long K; too small a buffer simply disables it), or the
        # per-tile row sums of a two-tile ln_out
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if ln_out is not None:         # (mean, rstd) of the output rows, for the next contraction's folded LayerNorm
        if ln_out.dtype != torch.float32 or tuple(ln_out.shape) != (m, 2) or not ln_out.is_contiguous():
            raise ValueError("ln_out must be a contiguous float32 [m][2] tensor")
        d.ln_out, d.ln_out_eps = ln_out.data_ptr(), float(ln_out_eps)
    d.w_group_rows, d.w_group_stride = int(w_group_rows), int(w_group_stride)
    if a2 is not None:                 # extra linear tap: rows of a second tensor against the weight's last cin2 columns
        _f16(a2, "a2")
        d.a2, d.lda2, d.cin2 = a2.data_ptr(), int(lda2 if lda2 is not None else a2.stride(0)), int(cin2)
    if gn_part is not None:            # fp32 [m/256][2][n][2]: per-tile column sums for the next GroupNorm (svdpipe.h)
        if gn_part.dtype != torch.float32 or not gn_part.is_cuda or gn_part.numel() < (m // 256) * 2 * n * 2:
            raise TypeError("gn_part must be a float32 HIP tensor of (m/256)*2*n*2 elements")
        d.gn_part = gn_part.data_ptr()
    taps = 9 if mode == A_CONV3X3 else 3 if mode == A_TEMPORAL3 else 1
    # algorithmic bytes of this launch: every operand element once (A without tap re-reads), output and residuals once
    a_rows = d.n_img * d.hin * d.win if mode == A_CONV3X3 else m
    k2 = int(cin2) if a2 is not None else 0          # (the extra linear tap's channels count like any other K)
    nbytes = 2.0 * (a_rows * cin + m * k2 + n * (taps * cin + k2) + m * (n_store or nout) * (1 + (res1 is not None) + (res2 is not None)))
    with _Timed("gemm", 2.0 * m * n * (taps * cin + k2), nbytes, (m, n, cin, mode, bool(geglu))) as tm:
        _check(load().sp_gemm_f16(ctypes.byref(d), _stream()), "sp_gemm_f16")
        if PROFILE is not None:      # which kernel template took it (per-template FLOPs in the profile summary)
            tm.tag = tm.tag + (load().sp_gemm_last_kernel().decode(),)
    return out


def _conv_up2x(a, w, out, *, m, n, cin, mode, lda, conv, bias, ldd, gn_part):
    """The ``up2x_phases`` leg of :func:`gemm`: same launch record (kind ``"gemm"``, same tag form), executed FLOPs."""
    if mode != A_CONV3X3 or conv is None or conv[-1] != 1 or conv[5] != 1:
        raise ValueError("gemm(up2x_phases=True) needs mode=A_CONV3X3 and an upsampling geometry (stride 1, upsample2x = 1)")
    n_img, hin, win, hout, wout = conv[:5]
    if (hout, wout) != (2 * hin, 2 * win) or m != n_img * hout * wout:
        raise ValueError(f"gemm(up2x_phases=True): m = {m}, output {hout}x{wout} do not match {n_img} images of {hin}x{win} doubled")
    if tuple(_f16(w, "w").shape) != (4, n, 4 * cin) or not w.is_contiguous():
        raise ValueError(f"gemm(up2x_phases=True): w must be the contiguous phase-major pack [4][{n}][{4 * cin}]; got {tuple(w.shape)}")
    lda = int(lda if lda is not None else cin)
    ldd = int(ldd if ldd is not None else n)
    _rows(a, "a", lda)
    _rows(out, "out", ldd)
    if gn_part is not None:            # fp32 [m/256][2][n][2], a frame's 4 * (hin*win/256) tiles contiguous (svdpipe.h)
        if gn_part.dtype != torch.float32 or not gn_part.is_cuda or gn_part.numel() < (m // 256) * 2 * n * 2:
            raise TypeError("gn_part must be a float32 HIP tensor of (m/256)*2*n*2 elements")
    # algorithmic bytes: every operand element once (the four phases' weights are 16*cin per output channel), output once
    nbytes = 2.0 * (n_img * hin * win * cin + n * 16 * cin + m * n)
    with _Timed("gemm", 2.0 * m * n * 4 * cin, nbytes, (m, n, cin, mode, False)) as tm:
        _check(load().sp_conv_up2x_f16(a.data_ptr(), lda, cin, n_img, hin, win, w.data_ptr(), n, _ptr(bias), out.data_ptr(),
                                       ldd, _ptr(gn_part), zero_page(a.device).data_ptr(), _stream()), "sp_conv_up2x_f16")
        if PROFILE is not None:
            tm.tag = tm.tag + (load().sp_gemm_last_kernel().decode(),)
    return out


def gemm_workspace_bytes(*, m, n, cin, mode=A_LINEAR) -> int:
    """Scratch bytes ``gemm(..., workspace=)`` can use for this shape (0: not a split-K candidate)."""
    d = GemmDesc()
    d.m, d.n, d.cin, d.mode = m, n, cin, mode
    return int(load().sp_gemm_workspace_bytes(ctypes.byref(d)))


class gemm_route:
    """``with gemm_route(3, bm=256): ...`` pins the kernel family of ``sp_gemm_f16`` (tests / micro-benchmarks only;
    see ``sp_gemm_set_route`` in include/svdpipe.h): 1 small tiles, 2 ping-pong, 3 persistent-stream."""

    def __init__(self, route: int, bm: int = 0, bn: int = 0):
        self.args = (route, bm, bn)

    def __enter__(self):
        _check(load().sp_gemm_set_route(*self.args), "sp_gemm_set_route")
        return self

    def __exit__(self, *exc):
        load().sp_gemm_set_route(0, 0, 0)
        return False


def gemv(x, w, b, *, n, k, rows=1, ldx=None, y32=None, y16=None, ldy=None, silu_in=False, silu_out=False):
    _check(load().sp_gemv_f16(_f16(x, "x").data_ptr(), int(ldx if ldx is not None else k), _f16(w, "w").data_ptr(),
                              _ptr(b), _ptr(y32), _ptr(y16), int(ldy if ldy is not None else n), rows, n, k,
                              int(silu_in), int(silu_out), _stream()), "sp_gemv_f16")


def gemv_batched(x, w, b, *, batch, n, k, rows=1, ldx=None, x_stride=None, y32=None, y16=None, ldy=None,
                 silu_in=False, silu_out=False):
    """``batch`` same-shape GEMVs in one launch: w [batch][n][k], b [batch][n] or None, y [batch][rows][n];
    x [batch][rows][k], or one shared [rows][k] input with ``x_stride=0``."""
    ldx = int(ldx if ldx is not None else k)
    ldy = int(ldy if ldy is not None else n)
    xs = int(rows * ldx if x_stride is None else x_stride)
    _check(load().sp_gemv_batched_f16(_f16(x, "x").data_ptr(), ldx, xs, _f16(w, "w").data_ptr(), n * k, _ptr(b), n,
                                      _ptr(y32), _ptr(y16), ldy, rows * ldy, batch, rows, n, k, int(silu_in),
                                      int(silu_out), _stream()), "sp_gemv_batched_f16")


def sinusoid(values32, out16, count, dim):
    _check(load().sp_sinusoid_f16(values32.data_ptr(), out16.data_ptr(), count, dim, _stream()), "sp_sinusoid_f16")


def groupnorm_ws_bytes(instances, rows, c, groups) -> int:
    return int(load().sp_groupnorm_ws_bytes(instances, rows, c, groups))


def groupnorm(x, gamma, beta, y, *, instances, rows, c, groups, eps, silu, ws, ldx=None):
    """``ldx``: halves between consecutive rows of ``x`` when it is a column slice of a wider tensor (default: dense)."""
    # algorithmic bytes: statistics pass reads x, apply pass reads x and writes y (the single-launch path reads once)
    with _Timed("groupnorm", 0.0, 3 * 2.0 * instances * rows * c):
        ldx = int(c if ldx is None else ldx)
        _check(load().sp_groupnorm_ld_f16(_rows(x, "x", ldx).data_ptr(), ldx, _ptr(gamma), _ptr(beta),
                                          _f16(y, "y").data_ptr(), instances, rows, c, groups, eps, int(silu),
                                          ws.data_ptr(), ws.numel() * ws.element_size(), _stream()), "sp_groupnorm_f16")
    return y


def groupnorm_tile_sums(x, part, gamma, beta, y, *, instances, rows, c, groups, eps, silu, stats, ldx=None, part_b=None,
                        c_a=None):
    """GroupNorm(+SiLU) of ``x`` from the per-tile column sums its producing contraction left in ``part``
    (``gemm(..., gn_part=part)``): no statistics pass over ``x`` (``sp_groupnorm_tile_sums_f16``).  ``part_b`` / ``c_a``: x is
    the concatenation of two producers' outputs, channels ``[0, c_a)`` summed in ``part``, the rest in ``part_b``."""
    ldx = int(ldx if ldx is not None else x.stride(0))
    with _Timed("groupnorm", 0.0, 2 * 2.0 * instances * rows * c):
        _check(load().sp_groupnorm_tile_sums2_f16(_f16(x, "x").data_ptr(), ldx, part.data_ptr(), int(c_a if part_b is not None else c),
                                                  _ptr(part_b), _ptr(gamma), _ptr(beta), _f16(y, "y").data_ptr(), instances, rows,
                                                  c, groups, float(eps), int(silu), stats.data_ptr(), _stream()),
               "sp_groupnorm_tile_sums2_f16")
    return y


def groupnorm_fold_linear_tile_sums(part, gamma, beta, w, bias, w_out, bias_out, *, instances, rows, c, groups, eps, n, stats):
    """``groupnorm_fold_linear`` with the statistics folded from a producer's per-tile column sums (``gemm(..., gn_part=)``)."""
    _check(load().sp_groupnorm_fold_linear_tile_sums_f16(part.data_ptr(), _ptr(gamma), _ptr(beta), instances, rows, c, groups,
                                                         float(eps), _f16(w, "w").data_ptr(), _ptr(bias), n,
                                                         _f16(w_out, "w_out").data_ptr(), bias_out.data_ptr(),
                                                         stats.data_ptr(), _stream()),
           "sp_groupnorm_fold_linear_tile_sums_f16")


def groupnorm_fold_linear(x, gamma, beta, w, bias, w_out, bias_out, *, instances, rows, c, groups, eps, n, ws, ldx=None):
    """GroupNorm (no activation) folded into the linear layer ``w`` [n][c] behind it: ONE pass over ``x`` (statistics) and
    ``w_out`` [instances][n][c] fp16 / ``bias_out`` [instances][n] fp32 for ``gemm(x, w_out, ..., w_group_rows=rows,
    w_group_stride=n*c, bias=None, bias2=bias_out, bias2_rows=rows)`` on the RAW ``x`` (see include/svdpipe.h)."""
    with _Timed("groupnorm", 0.0, 2.0 * instances * rows * c + 2.0 * instances * n * c):
        ldx = int(c if ldx is None else ldx)
        if tuple(w_out.shape) != (instances, n, c) or not w_out.is_contiguous() or bias_out.dtype != torch.float32 \
                or tuple(bias_out.shape) != (instances, n) or not bias_out.is_contiguous():
            raise ValueError("groupnorm_fold_linear: w_out must be contiguous fp16 [instances][n][c], bias_out fp32 [instances][n]")
        _check(load().sp_groupnorm_fold_linear_f16(_rows(x, "x", ldx).data_ptr(), ldx, _ptr(gamma), _ptr(beta), instances,
                                                   rows, c, groups, eps, _f16(w, "w").data_ptr(), _ptr(bias), n,
                                                   _f16(w_out, "w_out").data_ptr(), bias_out.data_ptr(), ws.data_ptr(),
                                                   ws.numel() * ws.element_size(), _stream()), "sp_groupnorm_fold_linear_f16")
    return w_out, bias_out


def layernorm(x, gamma, beta, y, *, rows, c, eps=1e-5, addvec=None, addvec_rows=0, sum_out=None):
    with _Timed("layernorm", 0.0, (2 + (sum_out is not None)) * 2.0 * rows * c):
        _check(load().sp_layernorm_f16(_f16(x, "x").data_ptr(), _ptr(addvec), addvec_rows, _ptr(sum_out),
                                       gamma.data_ptr(), beta.data_ptr(), _f16(y, "y").data_ptr(), rows, c, eps,
                                       _stream()), "sp_layernorm_f16")
    return y


def ln_stats(x, stats, *, rows, c, eps=1e-5, addvec=None, addvec_rows=0, sum_out=None):
    """Per-row (mean, rstd) of a LayerNorm that the next GEMM applies itself (``gemm(..., ln_stats=, ln_colsum=)``)."""
    with _Timed("ln_stats", 0.0, (1 + (sum_out is not None)) * 2.0 * rows * c + 8.0 * rows):
        _check(load().sp_ln_stats_f16(_f16(x, "x").data_ptr(), _ptr(addvec), addvec_rows, _ptr(sum_out),
                                      stats.data_ptr(), rows, c, eps, _stream()), "sp_ln_stats_f16")
    return stats


def attn_spatial(q, k, v, o, *, ldq, ldk, ldv, ldo, batch, seq, heads, scale=0.125):
    with _Timed("attn_spatial", 4.0 * batch * heads * seq * seq * 64):
        _check(load().sp_attn_spatial_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), ldq, ldk, ldv, ldo,
                                          batch, seq, heads, scale, zero_page(o.device).data_ptr(), _stream()),
               "sp_attn_spatial_f16")
    return o


def attn_long_ws_bytes(batch, seq, heads) -> int:
    return int(load().sp_attn_long_ws_bytes(batch, seq, heads))


def attn_spatial_long(q, k, v, o, workspace, *, ldq, ldk, ldv, ldo, batch, seq, heads, scale=0.125):
    """Spatial attention through the frozen-reference kernel for long rows (csrc/attention_long.hip; other shapes go to
    the ordinary kernel inside the call); `workspace`: tensor of >= attn_long_ws_bytes() bytes (flag words)."""
    long_rows = seq >= 4096 and seq % 256 == 0            # the call's own rule; other shapes run the ordinary kernel
    with _Timed("attn_spatial_long" if long_rows else "attn_spatial", 4.0 * batch * heads * seq * seq * 64):
        _check(load().sp_attn_spatial_long_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), ldq, ldk, ldv, ldo,
                                               batch, seq, heads, scale, zero_page(o.device).data_ptr(),
                                               workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                               _stream()),
               "sp_attn_spatial_long_f16")
    return o


def attn_long_set_occupancy(occ: int) -> None:
    """Pins the instantiation attn_spatial_long launches (1 or 2 workgroups per CU; 0 = the library's default):
    ``sp_attn_long_set_occupancy`` in include/svdpipe.h.  Tests and micro-benchmarks only."""
    _check(load().sp_attn_long_set_occupancy(occ), "sp_attn_long_set_occupancy")


def attn_long_last_kernel() -> str:
    return load().sp_attn_long_last_kernel().decode()


def attn_fp8_ws_bytes(batch, seq, heads) -> int:
    return int(load().sp_attn_fp8_ws_bytes(batch, seq, heads))


def attn_spatial_fp8(q, k, v, o, workspace, *, ldq, ldk, ldv, ldo, batch, seq, heads, scale=0.125):
    """fp8-e4m3 MFMA spatial attention (BASELINE config 5); `workspace`: uint8 tensor >= attn_fp8_ws_bytes()."""
    with _Timed("attn_spatial", 4.0 * batch * heads * seq * seq * 64):
        _check(load().sp_attn_spatial_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), ldq, ldk, ldv, ldo,
                                          batch, seq, heads, scale, workspace.data_ptr(),
                                          workspace.numel() * workspace.element_size(),
                                          zero_page(o.device).data_ptr(), _stream()),
               "sp_attn_spatial_fp8")
    return o


def attn_temporal(q, k, v, o, *, ldq, ldk, ldv, ldo, batch, frames, hw, heads, scale=0.125):
    with _Timed("attn_temporal", 4.0 * batch * hw * heads * frames * frames * 64, 4 * 2.0 * batch * frames * hw * heads * 64):
        _check(load().sp_attn_temporal_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), ldq, ldk, ldv, ldo,
                                           batch, frames, hw, heads, scale, zero_page(o.device).data_ptr(), _stream()),
               "sp_attn_temporal_f16")
    return o


def pack_input(latent, image_latents, out, *, in_scale, b, frames, h, w, cpad):
    _check(load().sp_pack_input_f16(_f16(latent, "latent").data_ptr(), _f16(image_latents, "image_latents").data_ptr(),
                                    out.data_ptr(), in_scale, b, frames, h, w, cpad, _stream()), "sp_pack_input_f16")
    return out


def softmax_rows(x, *, rows, cols, ld=None):
    """In-place softmax of every row of the fp16 matrix ``x`` (the VAE mid block's attention scores)."""
    ld = int(ld if ld is not None else cols)
    with _Timed("softmax_rows", 0.0, 2 * 2.0 * rows * cols):
        _check(load().sp_softmax_rows_f16(_rows(x, "x", ld).data_ptr(), ld, rows, cols, _stream()), "sp_softmax_rows_f16")
    return x


def gemm_f32out(a, w, out32, *, m, n, k, lda=None):
    """``out32[m][n]`` (fp32, contiguous) = ``a[m][k] @ w[n][k]^T`` as raw fp32 sums (``sp_gemm_f32out_f16``): logits that
    must not pass through fp16 on their way into a softmax.  n a multiple of 256, k of 64."""
    lda = int(lda if lda is not None else a.stride(0))
    _f16(a, "a"); _f16(w, "w")
    if out32.dtype != torch.float32 or not out32.is_cuda or not out32.is_contiguous() or out32.numel() < m * n:
        raise TypeError("out32 must be a contiguous float32 HIP tensor of at least m*n elements")
    if w.dim() == 2 and w.shape[0] > 1 and w.stride(0) != k:
        raise ValueError(f"w: row stride {w.stride(0)} must equal k = {k}")
    with _Timed("gemm_f32out", 2.0 * m * n * k, 2.0 * (m * k + n * k) + 4.0 * m * n):
        _check(load().sp_gemm_f32out_f16(a.data_ptr(), lda, w.data_ptr(), out32.data_ptr(), m, n, k,
                                         zero_page(a.device).data_ptr(), _stream()), "sp_gemm_f32out_f16")
    return out32


def softmax_rows_f32(x32, out16, *, rows, cols, scale=1.0, ld=None, ldo=None):
    """``out16[r][:cols] = fp16(softmax(scale * x32[r][:cols]))``, fp32 logits in, fp32 statistics (``sp_softmax_rows_f32``).
    ``out16`` may be a float16 VIEW of ``x32`` itself (``x32.view(torch.float16)``, row pitch 2*ld halves): the
    probabilities then overwrite the front of each row's logits."""
    ld = int(ld if ld is not None else x32.stride(0))
    ldo = int(ldo if ldo is not None else out16.stride(0))
    if x32.dtype != torch.float32 or not x32.is_cuda or out16.dtype != torch.float16 or not out16.is_cuda:
        raise TypeError("x32 must be float32 and out16 float16, both on a HIP device")
    with _Timed("softmax_rows", 0.0, (4.0 + 2.0) * rows * cols):
        _check(load().sp_softmax_rows_f32(x32.data_ptr(), ld, out16.data_ptr(), ldo, rows, cols, float(scale), _stream()),
               "sp_softmax_rows_f32")
    return out16


def softmax_rows_long_f32(x32, out16, *, rows, cols, scale=1.0, ld=None, ldo=None):
    """``softmax_rows_f32`` for rows of any length (``sp_softmax_rows_long_f32``): the row is streamed, not held in registers,
    so ``cols`` goes up to 2^24; up to 16,384 columns the bytes are ``softmax_rows_f32``'s.  In place as there."""
    ld = int(ld if ld is not None else x32.stride(0))
    ldo = int(ldo if ldo is not None else out16.stride(0))
    if x32.dtype != torch.float32 or not x32.is_cuda or out16.dtype != torch.float16 or not out16.is_cuda:
        raise TypeError("x32 must be float32 and out16 float16, both on a HIP device")
    with _Timed("softmax_rows", 0.0, (3 * 4.0 + 2.0) * rows * cols):
        _check(load().sp_softmax_rows_long_f32(x32.data_ptr(), ld, out16.data_ptr(), ldo, rows, cols, float(scale), _stream()),
               "sp_softmax_rows_long_f32")
    return out16


def video_strides(t, layout):
    """(sb, sc, sf) element strides of a contiguous video tensor: "bcfhw" = (B,C,F,H,W), "nchw" = (B*F,C,H,W)."""
    if layout == "bcfhw":
        _, c, f, h, w = t.shape
        return c * f * h * w, f * h * w, h * w
    _, c, h, w = t.shape
    return None, h * w, c * h * w          # sb = F*C*hw depends on the caller's frames per batch item


def vae_pack_latent(latent, rows, *, scale, flat0, n, frames_per_item, strides, h, w, cpad):
    sb, sc, sf = strides
    _check(load().sp_vae_pack_latent_f16(_f16(latent, "latent").data_ptr(), _f16(rows, "rows").data_ptr(), scale, flat0, n,
                                         frames_per_item, sb, sc, sf, h, w, cpad, _stream()), "sp_vae_pack_latent_f16")
    return rows


def vae_frames_out(rows, weight, bias, out, *, batch, frames, h, w, flat0, frames_per_item, strides):
    sb, sc, sf = strides
    if out.dtype not in (torch.float16, torch.float32) or not out.is_contiguous():
        raise TypeError("vae_frames_out: out must be a contiguous float16 or float32 tensor")
    with _Timed("vae_frames_out", 0.0, 2.0 * batch * frames * h * w * (rows.shape[1] + 3)):
        _check(load().sp_vae_frames_out_f16(_f16(rows, "rows").data_ptr(), rows.shape[1], weight.data_ptr(), bias.data_ptr(),
                                            out.data_ptr(), int(out.dtype == torch.float32), batch, frames, h, w, flat0,
                                            frames_per_item, sb, sc, sf, _stream()), "sp_vae_frames_out_f16")
    return out


def vae_frames_out_u8(rows, weight, bias, out, *, batch, frames, h, w, flat0):
    """time_conv_out of a decoder call stored as 8-bit frames: ``out`` is the dense (B*F, H, W, 3) uint8 video (any leading
    shape), the call writes entries flat0 .. flat0 + batch*frames - 1."""
    if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise TypeError("vae_frames_out_u8: out must be a contiguous uint8 tensor on a HIP device")
    if (flat0 + batch * frames) * h * w * 3 > out.numel():
        raise ValueError("vae_frames_out_u8: the call's entries do not fit in out")
    with _Timed("vae_frames_out", 0.0, batch * frames * h * w * (2.0 * rows.shape[1] + 3)):
        _check(load().sp_vae_frames_out_u8(_f16(rows, "rows").data_ptr(), rows.shape[1], weight.data_ptr(), bias.data_ptr(),
                                           out.data_ptr(), batch, frames, h, w, flat0, _stream()), "sp_vae_frames_out_u8")
    return out


def vae_image_pack(image, rows, *, batch, h, w, cpad, flip):
    _check(load().sp_vae_image_pack_f16(_f16(image, "image").data_ptr(), _f16(rows, "rows").data_ptr(), batch, h, w, cpad,
                                        int(flip), _stream()), "sp_vae_image_pack_f16")
    return rows


def vae_latent_out(rows, out, *, batch, channels, frames, h, w, flip):
    _check(load().sp_vae_latent_out_f16(_f16(rows, "rows").data_ptr(), rows.shape[1], _f16(out, "out").data_ptr(), batch,
                                        channels, frames, h, w, int(flip), _stream()), "sp_vae_latent_out_f16")
    return out


def patchify(pixels, rows, *, batch, h, w, patch, kpad):
    _check(load().sp_patchify_f16(_f16(pixels, "pixels").data_ptr(), _f16(rows, "rows").data_ptr(), batch, h, w, patch, kpad,
                                  _stream()), "sp_patchify_f16")
    return rows


def attn_small(q, k, v, o, *, ldq, ldk, ldv, ldo, batch, seq, heads, head_dim, scale):
    with _Timed("attn_small", 4.0 * batch * heads * seq * seq * head_dim):
        _check(load().sp_attn_small_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), ldq, ldk, ldv, ldo, batch, seq,
                                        heads, head_dim, scale, _stream()), "sp_attn_small_f16")
    return o


def gelu(x, y, *, quick=False):
    _check(load().sp_gelu_f16(_f16(x, "x").data_ptr(), _f16(y, "y").data_ptr(), x.numel(), int(quick), _stream()), "sp_gelu_f16")
    return y


FILTER_BICUBIC, FILTER_LANCZOS3 = 0, 1


def _image_u8(t: torch.Tensor, name: str) -> torch.Tensor:
    """Interleaved uint8 RGB (h, w, 3) on the device; rows may be any pitch >= 3*w bytes (a crop is a slice)."""
    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 3 or t.shape[2] != 3:
        raise TypeError(f"{name} must be a uint8 (h, w, 3) tensor on a HIP device")
    if t.stride(2) != 1 or (t.shape[1] > 1 and t.stride(1) != 3) or (t.shape[0] > 1 and t.stride(0) < 3 * t.shape[1]):
        raise ValueError(f"{name} must hold interleaved pixels in rows (strides (pitch, 3, 1)); got {tuple(t.stride())}")
    return t


def _pitch(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1]      # (the stride of a dimension of one is arbitrary)


def image_resample_tmp_bytes(src_h: int, dst_w: int) -> int:
    return int(load().sp_image_resample_tmp_bytes(src_h, dst_w))


def image_resample_u8(src, dst, tmp, *, filter):
    """Pillow's antialiased resize of ``src`` (h, w, 3) into ``dst`` (h', w', 3), both uint8 and possibly slices of larger
    images; ``tmp``: uint8 scratch of at least ``image_resample_tmp_bytes(h, w')`` bytes."""
    _image_u8(src, "src"), _image_u8(dst, "dst")
    if tmp.dtype != torch.uint8 or not tmp.is_cuda or not tmp.is_contiguous():
        raise TypeError("image_resample_u8: tmp must be a contiguous uint8 tensor on a HIP device")
    _check(load().sp_image_resample_u8(src.data_ptr(), _pitch(src), src.shape[0], src.shape[1], dst.data_ptr(), _pitch(dst),
                                       dst.shape[0], dst.shape[1], int(filter), tmp.data_ptr(), tmp.numel(), _stream()),
           "sp_image_resample_u8")
    return dst


def image_to_tensor(src, out, *, mean, std):
    """uint8 (h, w, 3) -> fp16 planar (3, h, w) = (v/255 - mean[c]) / std[c]; ``src`` may be a slice of a larger image."""
    _image_u8(src, "src")
    h, w = src.shape[0], src.shape[1]
    if not out.is_contiguous() or out.numel() != 3 * h * w:
        raise ValueError("image_to_tensor: out must be a contiguous tensor of 3*h*w values")
    m, s = [float(v) for v in mean], [float(v) for v in std]
    _check(load().sp_image_to_tensor_f16(src.data_ptr(), _pitch(src), h, w, _f16(out, "out").data_ptr(), m[0], m[1], m[2],
                                         s[0], s[1], s[2], _stream()), "sp_image_to_tensor_f16")
    return out


def frames_to_u8(frames, out):
    """(B, 3, F, H, W) fp16 / fp32 -> uint8 (B, F, H, W, 3): ((x + 1) / 2 * 255).clamp(0, 255), truncated; NaN gives 0."""
    if frames.dtype not in (torch.float16, torch.float32) or not frames.is_cuda or not frames.is_contiguous():
        raise TypeError("frames_to_u8: frames must be a contiguous float16 or float32 tensor on a HIP device")
    if frames.dim() != 5 or frames.shape[1] != 3:
        raise ValueError(f"frames_to_u8: frames must be (B, 3, F, H, W); got {tuple(frames.shape)}")
    b, _, f, h, w = frames.shape
    if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (b, f, h, w, 3):
        raise TypeError(f"frames_to_u8: out must be a contiguous uint8 tensor of shape {(b, f, h, w, 3)} on a HIP device")
    _check(load().sp_frames_to_u8(frames.data_ptr(), int(frames.dtype == torch.float32), out.data_ptr(), b, f, h, w, _stream()),
           "sp_frames_to_u8")
    return out


def jpeg_quant_tables(quality: int) -> tuple[bytes, bytes]:
    """``(luma, chroma)``: 64 bytes each in natural (row-major) order, libjpeg's scaling of the Annex K tables (host only)."""
    lu, ch = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
    _check(load().sp_jpeg_quant_tables(int(quality), ctypes.addressof(lu), ctypes.addressof(ch)), "sp_jpeg_quant_tables")
    return bytes(lu), bytes(ch)


def jpeg_huffman_table(which: int) -> tuple[bytes, bytes]:
    """``(bits, values)`` of Annex K table ``which`` (0 / 1: DC luminance / chrominance, 2 / 3: AC) as a DHT segment holds them."""
    bits, vals = (ctypes.c_uint8 * 16)(), (ctypes.c_uint8 * 162)()
    n = load().sp_jpeg_huffman_table(int(which), ctypes.addressof(bits), ctypes.addressof(vals))
    if n < 0:
        _check(n, "sp_jpeg_huffman_table")
    return bytes(bits), bytes(vals)[:n]


def jpeg_mcu_grid(h: int, w: int) -> tuple[int, int]:
    return (h + 15) // 16, (w + 15) // 16


def jpeg_coef_bytes(n: int, h: int, w: int) -> int:
    return int(load().sp_jpeg_coef_bytes(n, h, w))


def jpeg_stream_bytes(h: int, w: int, restart_mcus: int) -> int:
    return int(load().sp_jpeg_stream_bytes(h, w, restart_mcus))


def jpeg_entropy_ws_bytes(n: int, mcu_rows: int, mcu_cols: int, restart_mcus: int) -> int:
    return int(load().sp_jpeg_entropy_ws_bytes(n, mcu_rows, mcu_cols, restart_mcus))


def _dev_buf(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous {dtype} tensor on a HIP device")
    return t


def jpeg_dct_quant(frames_u8, coef, *, quality):
    """uint8 (n, h, w, 3) RGB -> int16 ``coef`` (n, mcu_rows, mcu_cols, 6, 64): quantised DCT coefficients of the 4:2:0 MCUs,
    blocks in zigzag order (``sp_jpeg_dct_quant_u8``)."""
    _dev_buf(frames_u8, torch.uint8, "jpeg_dct_quant: frames")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"jpeg_dct_quant: frames must be (n, h, w, 3); got {tuple(frames_u8.shape)}")
    n, h, w, _ = frames_u8.shape
    _dev_buf(coef, torch.int16, "jpeg_dct_quant: coef")
    if tuple(coef.shape) != (n, *jpeg_mcu_grid(h, w), 6, 64):
        raise ValueError(f"jpeg_dct_quant: coef must be {(n, *jpeg_mcu_grid(h, w), 6, 64)}; got {tuple(coef.shape)}")
    _check(load().sp_jpeg_dct_quant_u8(frames_u8.data_ptr(), n, h, w, int(quality), coef.data_ptr(), _stream()),
           "sp_jpeg_dct_quant_u8")
    return coef


def jpeg_entropy(coef, out, out_len, ws, *, restart_mcus):
    """int16 ``coef`` (n, mcu_rows, mcu_cols, 6, 64) -> the entropy-coded segment of frame i in ``out[i, :out_len[i]]``
    (``out``: uint8 (n, cap), cap >= ``jpeg_stream_bytes``; ``out_len``: int32 (n,); ``ws``: uint8 scratch of
    ``jpeg_entropy_ws_bytes``)."""
    _dev_buf(coef, torch.int16, "jpeg_entropy: coef")
    if coef.dim() != 5 or tuple(coef.shape[3:]) != (6, 64):
        raise ValueError(f"jpeg_entropy: coef must be (n, mcu_rows, mcu_cols, 6, 64); got {tuple(coef.shape)}")
    n, mcu_rows, mcu_cols = coef.shape[:3]
    _dev_buf(out, torch.uint8, "jpeg_entropy: out"), _dev_buf(ws, torch.uint8, "jpeg_entropy: ws")
    _dev_buf(out_len, torch.int32, "jpeg_entropy: out_len")
    if out.dim() != 2 or out.shape[0] != n or out_len.numel() != n:
        raise ValueError("jpeg_entropy: out must be (n, cap) and out_len (n,)")
    _check(load().sp_jpeg_entropy(coef.data_ptr(), n, mcu_rows, mcu_cols, int(restart_mcus), out.data_ptr(), out.shape[1],
                                  out_len.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sp_jpeg_entropy")
    return out, out_len


def jpeg_decode_plan(fields, quant, have_quant: int, bits, vals, have_huff: int) -> bytes:
    """The plan of one baseline JPEG (``sp_jpeg_decode_plan``, host only): ``fields`` 17 ints, ``quant`` 4 x 64 bytes in natural
    order, ``bits`` 4 x 16 and ``vals`` 4 x 256 bytes (DC 0, DC 1, AC 0, AC 1), ``have_*`` the bit sets of the tables defined.
    ``ValueError`` with the library's reason for what it refuses."""
    if len(fields) != 17 or len(quant) != 256 or len(bits) != 64 or len(vals) != 1024:
        raise ValueError("jpeg_decode_plan: fields holds 17 ints, quant 256, bits 64 and vals 1024 bytes")
    f = (ctypes.c_int32 * 17)(*[int(v) for v in fields])
    q, b, v = (ctypes.c_uint8 * 256).from_buffer_copy(bytes(quant)), (ctypes.c_uint8 * 64).from_buffer_copy(bytes(bits)), \
        (ctypes.c_uint8 * 1024).from_buffer_copy(bytes(vals))
    lib = load()
    plan = ctypes.create_string_buffer(lib.sp_jpeg_decode_plan_bytes())
    if lib.sp_jpeg_decode_plan(ctypes.addressof(f), ctypes.addressof(q), int(have_quant), ctypes.addressof(b), ctypes.addressof(v),
                               int(have_huff), ctypes.addressof(plan)) != 0:
        raise ValueError(last_error())
    return plan.raw


class JpegPlan:
    """A plan in host memory (kept alive here) next to its copy on the device: what the four decode calls take."""

    def __init__(self, plan: bytes, plan_dev: torch.Tensor) -> None:
        self.host = ctypes.create_string_buffer(plan, len(plan))
        _dev_buf(plan_dev, torch.uint8, "JpegPlan: plan_dev")
        if plan_dev.numel() < len(plan):
            raise ValueError("JpegPlan: plan_dev is shorter than the plan")
        self.dev = plan_dev
        self.ws_bytes = int(load().sp_jpeg_decode_ws_bytes(ctypes.addressof(self.host)))
        self.coef_bytes = int(load().sp_jpeg_decode_coef_bytes(ctypes.addressof(self.host)))

    @property
    def ptr(self) -> int:
        return ctypes.addressof(self.host)


def jpeg_decode_plan_bytes() -> int:
    return int(load().sp_jpeg_decode_plan_bytes())


def jpeg_decode_split(plan: JpegPlan, segment, ws):
    """Stage 1 (``sp_jpeg_decode_split``): ``segment`` uint8 device bytes of the entropy-coded segment, ``ws`` uint8 scratch of
    ``plan.ws_bytes`` whose first 64 int32 are the status block."""
    _dev_buf(segment, torch.uint8, "jpeg_decode_split: segment"), _dev_buf(ws, torch.uint8, "jpeg_decode_split: ws")
    _check(load().sp_jpeg_decode_split(plan.ptr, plan.dev.data_ptr(), segment.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
           "sp_jpeg_decode_split")


def jpeg_decode_sync(plan: JpegPlan, ws, first_pass: int, passes: int):
    """Stage 2 (``sp_jpeg_decode_sync``): synchronisation passes ``first_pass .. first_pass + passes - 1``."""
    _dev_buf(ws, torch.uint8, "jpeg_decode_sync: ws")
    _check(load().sp_jpeg_decode_sync(plan.ptr, plan.dev.data_ptr(), ws.data_ptr(), ws.numel(), int(first_pass), int(passes),
                                      _stream()), "sp_jpeg_decode_sync")


def jpeg_decode_coefficients(plan: JpegPlan, ws, last_pass: int, coef):
    """Stage 3 (``sp_jpeg_decode_coefficients``): ``coef`` int16 of ``plan.coef_bytes``; nothing happens before the fixed point."""
    _dev_buf(ws, torch.uint8, "jpeg_decode_coefficients: ws"), _dev_buf(coef, torch.int16, "jpeg_decode_coefficients: coef")
    if coef.numel() * 2 != plan.coef_bytes:
        raise ValueError(f"jpeg_decode_coefficients: coef must hold {plan.coef_bytes} bytes; got {coef.numel() * 2}")
    _check(load().sp_jpeg_decode_coefficients(plan.ptr, plan.dev.data_ptr(), ws.data_ptr(), ws.numel(), int(last_pass),
                                              coef.data_ptr(), _stream()), "sp_jpeg_decode_coefficients")
    return coef


def jpeg_decode_pixels(plan: JpegPlan, ws, coef, rgb):
    """Stage 4 (``sp_jpeg_decode_pixels``): ``coef`` -> ``rgb`` uint8 (h, w, 3)."""
    _dev_buf(ws, torch.uint8, "jpeg_decode_pixels: ws"), _dev_buf(coef, torch.int16, "jpeg_decode_pixels: coef")
    _dev_buf(rgb, torch.uint8, "jpeg_decode_pixels: rgb")
    if coef.numel() * 2 != plan.coef_bytes or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError("jpeg_decode_pixels: coef must hold plan.coef_bytes and rgb be (h, w, 3)")
    _check(load().sp_jpeg_decode_pixels(plan.ptr, plan.dev.data_ptr(), ws.data_ptr(), ws.numel(), coef.data_ptr(), rgb.data_ptr(),
                                        _stream()), "sp_jpeg_decode_pixels")
    return rgb


def gif_ws_bytes(n: int, h: int, w: int, strip_rows: int) -> int:
    return int(load().sp_gif_ws_bytes(n, h, w, strip_rows))


def gif_stream_bytes(h: int, w: int, strip_rows: int) -> int:
    return int(load().sp_gif_stream_bytes(h, w, strip_rows))


def gif_quantise(frames_u8, palette, indices, ws):
    """uint8 (n, h, w, 3) RGB -> ``palette`` uint8 (n, 256, 3) and ``indices`` uint8 (n, h, w): a median-cut palette of every
    frame over a 32^3 histogram and the nearest entry per occupied bin (``sp_gif_quantise_u8``); ``ws``: uint8 scratch of
    ``gif_ws_bytes``."""
    _dev_buf(frames_u8, torch.uint8, "gif_quantise: frames")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"gif_quantise: frames must be (n, h, w, 3); got {tuple(frames_u8.shape)}")
    n, h, w, _ = frames_u8.shape
    _dev_buf(palette, torch.uint8, "gif_quantise: palette"), _dev_buf(indices, torch.uint8, "gif_quantise: indices")
    _dev_buf(ws, torch.uint8, "gif_quantise: ws")
    if tuple(palette.shape) != (n, 256, 3) or tuple(indices.shape) != (n, h, w):
        raise ValueError(f"gif_quantise: palette must be {(n, 256, 3)} and indices {(n, h, w)}; got {tuple(palette.shape)} and "
                         f"{tuple(indices.shape)}")
    _check(load().sp_gif_quantise_u8(frames_u8.data_ptr(), n, h, w, palette.data_ptr(), indices.data_ptr(), ws.data_ptr(),
                                     ws.numel(), _stream()), "sp_gif_quantise_u8")
    return palette, indices


def gif_lzw(indices, out, out_len, ws, *, strip_rows):
    """uint8 ``indices`` (n, h, w) -> the image data of frame i's GIF image block in ``out[i, :out_len[i]]`` (``out``: uint8
    (n, cap), cap >= ``gif_stream_bytes``; ``out_len``: int32 (n,); ``ws``: uint8 scratch of ``gif_ws_bytes``)."""
    _dev_buf(indices, torch.uint8, "gif_lzw: indices")
    if indices.dim() != 3:
        raise ValueError(f"gif_lzw: indices must be (n, h, w); got {tuple(indices.shape)}")
    n, h, w = indices.shape
    _dev_buf(out, torch.uint8, "gif_lzw: out"), _dev_buf(ws, torch.uint8, "gif_lzw: ws")
    _dev_buf(out_len, torch.int32, "gif_lzw: out_len")
    if out.dim() != 2 or out.shape[0] != n or out_len.numel() != n:
        raise ValueError("gif_lzw: out must be (n, cap) and out_len (n,)")
    _check(load().sp_gif_lzw(indices.data_ptr(), n, h, w, int(strip_rows), out.data_ptr(), out.shape[1], out_len.data_ptr(),
                             ws.data_ptr(), ws.numel(), _stream()), "sp_gif_lzw")
    return out, out_len


def png_ws_bytes(n: int, h: int, w: int, strip_rows: int) -> int:
    return int(load().sp_png_ws_bytes(n, h, w, strip_rows))


def png_stream_bytes(h: int, w: int, strip_rows: int) -> int:
    return int(load().sp_png_stream_bytes(h, w, strip_rows))


def png_filter(frames_u8, filtered):
    """uint8 (n, h, w, 3) RGB -> ``filtered`` uint8 (n, h, 1 + 3w): every row behind the PNG filter type that gives the least
    sum of min(b, 256 - b) (``sp_png_filter_u8``)."""
    _dev_buf(frames_u8, torch.uint8, "png_filter: frames")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"png_filter: frames must be (n, h, w, 3); got {tuple(frames_u8.shape)}")
    n, h, w, _ = frames_u8.shape
    _dev_buf(filtered, torch.uint8, "png_filter: filtered")
    if tuple(filtered.shape) != (n, h, 1 + 3 * w):
        raise ValueError(f"png_filter: filtered must be {(n, h, 1 + 3 * w)}; got {tuple(filtered.shape)}")
    _check(load().sp_png_filter_u8(frames_u8.data_ptr(), n, h, w, filtered.data_ptr(), _stream()), "sp_png_filter_u8")
    return filtered


def png_deflate(filtered, out, out_len, ws, *, strip_rows):
    """uint8 ``filtered`` (n, h, 1 + 3w) -> frame i's complete zlib stream in ``out[i, :out_len[i]]`` (``out``: uint8 (n, cap),
    cap >= ``png_stream_bytes``; ``out_len``: int32 (n,); ``ws``: uint8 scratch of ``png_ws_bytes``)."""
    _dev_buf(filtered, torch.uint8, "png_deflate: filtered")
    if filtered.dim() != 3 or filtered.shape[2] < 4 or (filtered.shape[2] - 1) % 3:
        raise ValueError(f"png_deflate: filtered must be (n, h, 1 + 3w); got {tuple(filtered.shape)}")
    n, h, pitch = filtered.shape
    _dev_buf(out, torch.uint8, "png_deflate: out"), _dev_buf(ws, torch.uint8, "png_deflate: ws")
    _dev_buf(out_len, torch.int32, "png_deflate: out_len")
    if out.dim() != 2 or out.shape[0] != n or out_len.numel() != n:
        raise ValueError("png_deflate: out must be (n, cap) and out_len (n,)")
    _check(load().sp_png_deflate(filtered.data_ptr(), n, h, (pitch - 1) // 3, int(strip_rows), out.data_ptr(), out.shape[1],
                                 out_len.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sp_png_deflate")
    return out, out_len


def png_file_bytes(h: int, w: int, strip_rows: int) -> int:
    return int(load().sp_png_file_bytes(h, w, strip_rows))


def apng_file_bytes(n: int, h: int, w: int, strip_rows: int) -> int:
    return int(load().sp_apng_file_bytes(n, h, w, strip_rows))


def png_wrap_ws_bytes(n: int, cap: int) -> int:
    return int(load().sp_png_wrap_ws_bytes(n, cap))


def png_wrap(streams, lens, files, file_len, ws, *, height, width, animate=False, delay=(1, 7)):
    """The zlib streams ``streams[i, :lens[i]]`` (uint8 (n, cap), int32 (n,): what ``png_deflate`` leaves) -> complete files on
    the device (``sp_png_wrap``).  ``animate`` false: ``files`` is uint8 (n, file_cap), file_cap >= cap + 57, and row i one still
    of ``file_len[i]`` bytes; true: ``files`` is one uint8 buffer of at least 65 + n (50 + cap) + 4 (n - 1) bytes that receives one
    animated PNG of ``file_len[0]`` bytes, ``delay`` = (numerator, denominator) seconds per frame.  ``file_len``: int32 (n,);
    ``ws``: uint8 scratch of ``png_wrap_ws_bytes``."""
    _dev_buf(streams, torch.uint8, "png_wrap: streams"), _dev_buf(files, torch.uint8, "png_wrap: files")
    _dev_buf(lens, torch.int32, "png_wrap: lens"), _dev_buf(file_len, torch.int32, "png_wrap: file_len")
    _dev_buf(ws, torch.uint8, "png_wrap: ws")
    if streams.dim() != 2 or lens.numel() != streams.shape[0] or file_len.numel() != streams.shape[0]:
        raise ValueError("png_wrap: streams must be (n, cap), lens and file_len (n,)")
    n, cap = streams.shape
    if animate:
        if files.dim() != 1:
            raise ValueError(f"png_wrap: an animation's files must be one flat buffer; got {tuple(files.shape)}")
        file_cap = files.numel()
    else:
        if files.dim() != 2 or files.shape[0] != n:
            raise ValueError(f"png_wrap: files must be (n, file_cap); got {tuple(files.shape)}")
        file_cap = files.shape[1]
    _check(load().sp_png_wrap(streams.data_ptr(), cap, lens.data_ptr(), n, int(height), int(width), 1 if animate else 0,
                              int(delay[0]), int(delay[1]), files.data_ptr(), file_cap, file_len.data_ptr(), ws.data_ptr(),
                              ws.numel(), _stream()), "sp_png_wrap")
    return files, file_len


def crc32_ws_bytes(n: int, pitch: int) -> int:
    return int(load().sp_crc32_ws_bytes(n, pitch))


_WORD32 = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)


def crc32_rows(data, lens, crc, ws, seed=None):
    """``crc[i] = zlib.crc32(data[i, :lens[i]], seed[i])`` on the device (``sp_crc32_rows``).  ``data``: uint8 (n, pitch), any
    pitch; ``lens``: int32 (n,), read on the device (below 0 counts as 0, above pitch as pitch); ``seed``: (n,) 32-bit words or
    ``None`` for 0; ``crc``: (n,) 32-bit words (``torch.int32`` holds the bit pattern, ``torch.uint32`` is taken too); ``ws``:
    uint8 scratch of ``crc32_ws_bytes``."""
    _dev_buf(data, torch.uint8, "crc32_rows: data"), _dev_buf(lens, torch.int32, "crc32_rows: lens")
    _dev_buf(ws, torch.uint8, "crc32_rows: ws")
    if data.dim() != 2 or lens.numel() != data.shape[0]:
        raise ValueError("crc32_rows: data must be (n, pitch) and lens (n,)")
    n, pitch = data.shape
    for name, t in (("crc", crc), ("seed", seed)):
        if t is None and name == "seed":
            continue
        if t.dtype not in _WORD32 or not t.is_cuda or not t.is_contiguous() or t.numel() < n:
            raise TypeError(f"crc32_rows: {name} must be a contiguous tensor of n 32-bit words on a HIP device")
    _check(load().sp_crc32_rows(data.data_ptr(), pitch, lens.data_ptr(), _ptr(seed), n, crc.data_ptr(), ws.data_ptr(), ws.numel(),
                                _stream()), "sp_crc32_rows")
    return crc


def webp_ws_bytes(n: int, h: int, w: int, pred_bits: int, group_bits: int) -> int:
    return int(load().sp_webp_ws_bytes(n, h, w, pred_bits, group_bits))


def webp_stream_bytes(h: int, w: int, pred_bits: int, group_bits: int) -> int:
    return int(load().sp_webp_stream_bytes(h, w, pred_bits, group_bits))


def webp_transform(frames_u8, residual, modes, flags, ws, *, pred_bits):
    """uint8 (n, h, w, 3) RGB -> ``flags`` int32 (n,): subtract green or not; ``modes`` uint8 (n, bh, bw): the predictor of every
    block of 2^pred_bits pixels square; ``residual`` uint8 (n, h, w, 4): the residual bytes B, G, R, 0 (``sp_webp_transform_u8``)."""
    _dev_buf(frames_u8, torch.uint8, "webp_transform: frames")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"webp_transform: frames must be (n, h, w, 3); got {tuple(frames_u8.shape)}")
    n, h, w, _ = frames_u8.shape
    pred_bits = int(pred_bits)
    if not 2 <= pred_bits <= 9:
        raise ValueError(f"webp_transform: pred_bits must be 2..9; got {pred_bits}")
    bh, bw = -(-h // (1 << pred_bits)), -(-w // (1 << pred_bits))
    _dev_buf(residual, torch.uint8, "webp_transform: residual"), _dev_buf(modes, torch.uint8, "webp_transform: modes")
    _dev_buf(flags, torch.int32, "webp_transform: flags"), _dev_buf(ws, torch.uint8, "webp_transform: ws")
    if tuple(residual.shape) != (n, h, w, 4) or tuple(modes.shape) != (n, bh, bw) or flags.numel() != n:
        raise ValueError(f"webp_transform: residual must be {(n, h, w, 4)}, modes {(n, bh, bw)} and flags ({n},); got "
                         f"{tuple(residual.shape)}, {tuple(modes.shape)} and {tuple(flags.shape)}")
    _check(load().sp_webp_transform_u8(frames_u8.data_ptr(), n, h, w, pred_bits, residual.data_ptr(), modes.data_ptr(),
                                       flags.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sp_webp_transform_u8")
    return residual, modes, flags


def webp_code(residual, modes, flags, out, out_len, ws, *, pred_bits, group_bits):
    """The transform's outputs -> frame i's complete VP8L stream in ``out[i, :out_len[i]]`` (``out``: uint8 (n, cap), cap >=
    ``webp_stream_bytes``; ``out_len``: int32 (n,); ``ws``: uint8 scratch of ``webp_ws_bytes``)."""
    _dev_buf(residual, torch.uint8, "webp_code: residual")
    if residual.dim() != 4 or residual.shape[3] != 4:
        raise ValueError(f"webp_code: residual must be (n, h, w, 4); got {tuple(residual.shape)}")
    n, h, w, _ = residual.shape
    pred_bits, group_bits = int(pred_bits), int(group_bits)
    if not 2 <= pred_bits <= 9 or not (group_bits == 0 or 2 <= group_bits <= 9):
        raise ValueError(f"webp_code: pred_bits must be 2..9 and group_bits 0 or 2..9; got {pred_bits} and {group_bits}")
    bh, bw = -(-h // (1 << pred_bits)), -(-w // (1 << pred_bits))
    _dev_buf(modes, torch.uint8, "webp_code: modes"), _dev_buf(flags, torch.int32, "webp_code: flags")
    _dev_buf(out, torch.uint8, "webp_code: out"), _dev_buf(ws, torch.uint8, "webp_code: ws")
    _dev_buf(out_len, torch.int32, "webp_code: out_len")
    if tuple(modes.shape) != (n, bh, bw) or flags.numel() != n:
        raise ValueError(f"webp_code: modes must be {(n, bh, bw)} and flags ({n},); got {tuple(modes.shape)} and {tuple(flags.shape)}")
    if out.dim() != 2 or out.shape[0] != n or out_len.numel() != n:
        raise ValueError("webp_code: out must be (n, cap) and out_len (n,)")
    _check(load().sp_webp_code(residual.data_ptr(), modes.data_ptr(), flags.data_ptr(), n, h, w, pred_bits, group_bits,
                               out.data_ptr(), out.shape[1], out_len.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
           "sp_webp_code")
    return out, out_len


def interp_ws_bytes(n: int, h: int, w: int, search_range: int) -> int:
    return int(load().sp_interp_ws_bytes(n, h, w, search_range))


def _interp_frames(frames_u8, name: str):
    _dev_buf(frames_u8, torch.uint8, f"{name}: frames")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"{name}: frames must be (n, h, w, 3); got {tuple(frames_u8.shape)}")
    return frames_u8.shape[:3]


def interp_motion(frames_u8, vectors, ws, *, search_range, penalty, raw_vectors=None):
    """uint8 (n, h, w, 3) RGB -> ``vectors`` int16 (n - 1, h / 8, w / 8, 2), (vy, vx) per 8x8 block of each pair's midpoint:
    the exhaustive bilateral search over [-search_range, search_range]^2 on luma with ``penalty`` per unit of |vy| + |vx|,
    then the 3x3 median (``sp_interp_motion_u8``); ``raw_vectors``, if given, takes the vectors before the median; ``ws``:
    uint8 scratch of ``interp_ws_bytes``."""
    n, h, w = _interp_frames(frames_u8, "interp_motion")
    shape = (n - 1, h // 8, w // 8, 2)
    for t, what in ((vectors, "vectors"), (raw_vectors, "raw_vectors")):
        if t is None:
            continue
        _dev_buf(t, torch.int16, f"interp_motion: {what}")
        if tuple(t.shape) != shape:
            raise ValueError(f"interp_motion: {what} must be {shape}; got {tuple(t.shape)}")
    _dev_buf(ws, torch.uint8, "interp_motion: ws")
    _check(load().sp_interp_motion_u8(frames_u8.data_ptr(), n, h, w, int(search_range), int(penalty), vectors.data_ptr(),
                                      _ptr(raw_vectors), ws.data_ptr(), ws.numel(), _stream()), "sp_interp_motion_u8")
    return vectors


def interp_compensate(frames_u8, vectors, out):
    """uint8 (n, h, w, 3) and int16 ``vectors`` (n - 1, h / 8, w / 8, 2) -> ``out`` uint8 (2n - 1, h, w, 3): ``out[2i]`` is frame
    i, ``out[2i + 1]`` the overlapped, motion-compensated blend of frames i and i + 1 (``sp_interp_compensate_u8``)."""
    n, h, w = _interp_frames(frames_u8, "interp_compensate")
    _dev_buf(vectors, torch.int16, "interp_compensate: vectors"), _dev_buf(out, torch.uint8, "interp_compensate: out")
    if tuple(vectors.shape) != (n - 1, h // 8, w // 8, 2) or tuple(out.shape) != (2 * n - 1, h, w, 3):
        raise ValueError(f"interp_compensate: vectors must be {(n - 1, h // 8, w // 8, 2)} and out {(2 * n - 1, h, w, 3)}; got "
                         f"{tuple(vectors.shape)} and {tuple(out.shape)}")
    _check(load().sp_interp_compensate_u8(frames_u8.data_ptr(), n, h, w, vectors.data_ptr(), out.data_ptr(), _stream()),
           "sp_interp_compensate_u8")
    return out


class ClockStamps:
    """Stamps of the shader-clock counter against the constant 100 MHz counter, taken in stream order between other work
    (``sp_clock_stamp``; bench.py ``roofline.clock_ghz_live``).  ``stamp()`` enqueues one on the current stream (a 3 us
    launch of 1,024 one-wave workgroups, four a CU on average, each noting where it ran: the XCD in bits 3:0 of its id, the CU above
    them); ``ghz()`` (after a synchronise) pairs the first and the last stamp CU by CU -- the counters of two CUs need not
    share an origin, not even within one XCD, and a launch of fewer workgroups than CUs lands on other CUs every time --
    takes each XCD's median CU and returns (GHz, seconds between the stamps, XCDs seen in both) -- the shader clock the
    chip held over that stretch -- or None with fewer than two stamps or no CU in both.  Measured: profiles/clock_stamp_per_cu.txt."""
    BLOCKS = 1024

    def __init__(self, device, capacity):
        import torch
        self.buf = torch.zeros((capacity, self.BLOCKS, 4), dtype=torch.int64, device=device)
        self.n = 0

    def stamp(self):
        if self.n < self.buf.shape[0]:
            _check(load().sp_clock_stamp(self.buf[self.n].data_ptr(), self.BLOCKS, _stream()), "sp_clock_stamp")
            self.n += 1

    def ghz(self):
        if self.n < 2:
            return None
        b = self.buf[:self.n].cpu()
        real = b[:, :, 2].double().mean(dim=1)                 # when each stamp ran (its workgroups: within microseconds)
        first, last = b[int(real.argmin())], b[int(real.argmax())]
        per_xcd = {}
        rows = [{r[0]: r for r in reversed(stamp.tolist())} for stamp in (first, last)]      # a CU's first workgroup
        for place in sorted(rows[0].keys() & rows[1].keys()):
            f, l = rows[0][place], rows[1][place]
            dr = l[2] - f[2]
            if dr > 0:
                per_xcd.setdefault(place & 15, []).append((0.1 * (l[1] - f[1]) / dr, dr / 1e8))
        if not per_xcd:
            return None
        mid = [sorted(pairs)[len(pairs) // 2] for pairs in per_xcd.values()]
        return sum(r for r, _ in mid) / len(mid), sum(s for _, s in mid) / len(mid), len(mid)


def _seeds(seeds, batch: int, name: str):
    """The per-video noise seeds of a stochastic tail: int64 ``[batch]`` on the device (the kernels read them as uint64)."""
    if seeds.dtype != torch.int64 or not seeds.is_cuda or seeds.shape != (batch,) or not seeds.is_contiguous():
        raise ValueError(f"{name}: seeds must be a contiguous int64 [{batch}] tensor on the HIP device; got {seeds.dtype} "
                         f"{tuple(seeds.shape)}")
    return seeds.data_ptr()


def _tail(entry, name, stepped, *, channels, batch, dims, patch, eps, guidance, ld_eps, ld_guidance, consts, rest=(), lead=(),
          weights=None, noise=None):
    """One sampler-tail call ``entry(*lead, input, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, output, *consts, batch,
    *rest[, noise_scale, seeds, step], stream)`` behind the checks of what the kernels cannot see through raw pointers.
    ``stepped``: name -> tensor of the stepped tensor and of its output, each contiguous ``(batch, channels, *dims)`` with
    ``dims = (frames_total, h, w)``; ``patch = (n_patch, window, tile_h, tile_w)``: the eps buffers hold
    ``[n_patch][B][window][tile_h*tile_w][ld_eps]``; ``weights``: the ``[n_patch][window]`` table of an entry that takes frame
    windows as arguments; ``noise = (noise_scale, seeds, step)`` of an entry that takes them."""
    n_patch, window, tile_h, tile_w = patch
    eps_cond, eps_uncond = eps
    for what, t in stepped.items():
        if _f16(t, what).shape != (batch, channels, *dims) or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be a contiguous ({batch}, {channels}, {dims[0]}, {dims[1]}, {dims[2]}) tensor; "
                             f"got {tuple(t.shape)}, strides {tuple(t.stride())}")
    for what, t in (("eps_cond", eps_cond), ("eps_uncond", eps_uncond)):
        if t is not None and (_f16(t, what).numel() != n_patch * batch * window * tile_h * tile_w * ld_eps or not t.is_contiguous()):
            raise ValueError(f"{name}: {what} must hold [n_patch={n_patch}][B={batch}][window={window}][{tile_h * tile_w}]"
                             f"[ld_eps={ld_eps}] contiguous values; got {tuple(t.shape)}")
    if weights is not None and (weights.dtype != torch.float32 or weights.numel() != n_patch * window or not weights.is_contiguous()):
        raise ValueError(f"{name}: weights must be a contiguous float32 [{n_patch}][{window}] table; got {weights.dtype} "
                         f"{tuple(weights.shape)}")
    if noise is not None:
        noise_scale, seeds, step = noise
        if seeds is None and noise_scale != 0.0:
            raise ValueError(f"{name}: noise_scale={noise_scale} needs the videos' seeds")
        rest = (*rest, noise_scale, None if seeds is None else _seeds(seeds, batch, name), int(step))
    src, out = stepped.values()
    _check(getattr(load(), entry)(*lead, src.data_ptr(), eps_cond.data_ptr(), _ptr(eps_uncond), ld_eps, _ptr(guidance),
                                  int(ld_guidance), out.data_ptr(), *consts, batch, *rest, _stream()), entry)
    return out


def _windows(frames_total, h, w, window, stride, n_win, weights):
    """``(patch, rest)`` of an entry that takes frame windows as arguments; ``weights=None``: one window that is the whole latent."""
    if weights is None:
        window, stride, n_win = frames_total, frames_total, 1
    return (n_win, window, h, w), (frames_total, h, w, window, stride, n_win, _ptr(weights))


def euler_step(latent, eps_cond, eps_uncond, guidance, out, *, ld_eps, sigma, sigma_next, b, frames, h, w,
               ld_guidance=0):
    """``ld_guidance``: ``guidance`` is fp32 [B][ld_guidance], one row of per-frame scales per video; 0 = one [F] row
    shared by every video (``sp_euler_step_rows_f16``)."""
    return _tail("sp_euler_step_rows_f16", "euler_step", {"latent": latent, "out": out}, channels=4, batch=b, dims=(frames, h, w),
                 patch=(1, frames, h, w), eps=(eps_cond, eps_uncond), guidance=guidance, ld_eps=ld_eps, ld_guidance=ld_guidance,
                 consts=(sigma, sigma_next), rest=(frames, h, w))


def dpmpp2m_step(state, eps_cond, eps_uncond, guidance, out_state, *, ld_eps, sigma, a, b, c1, c2, batch, frames, h, w,
                 ld_guidance=0):
    """DPM-Solver++(2M) update of the 8-channel ``state`` (B,8,F,H,W: sample ++ previous denoised estimate) into
    ``out_state`` (may be ``state`` itself); ``guidance`` / ``ld_guidance`` as for ``euler_step``
    (``sp_dpmpp2m_step_rows_f16``)."""
    return _tail("sp_dpmpp2m_step_rows_f16", "dpmpp2m_step", {"state": state, "out_state": out_state}, channels=8, batch=batch,
                 dims=(frames, h, w), patch=(1, frames, h, w), eps=(eps_cond, eps_uncond), guidance=guidance, ld_eps=ld_eps, ld_guidance=ld_guidance,
                 consts=(sigma, a, b, c1, c2), rest=(frames, h, w))


def euler_step_windows(latent, eps_cond, eps_uncond, guidance, out, *, ld_eps, sigma, sigma_next, b, frames_total, h, w,
                       window, stride, n_win, weights, ld_guidance=0):
    """The Euler update of ``latent`` (B,4,F_total,H,W) behind the eps rows of ``n_win`` overlapping frame windows
    (``[n_win][B][window][H*W][ld_eps]``), blended with ``weights`` (fp32 ``[n_win][window]``, ``models.window_plan.plan``);
    ``guidance`` is indexed by the position in the window (``sp_euler_step_windows_f16``)."""
    patch, rest = _windows(frames_total, h, w, window, stride, n_win, weights)
    return _tail("sp_euler_step_windows_f16", "euler_step_windows", {"latent": latent, "out": out}, channels=4, batch=b,
                 dims=(frames_total, h, w), patch=patch, eps=(eps_cond, eps_uncond), guidance=guidance, ld_eps=ld_eps, ld_guidance=ld_guidance,
                 consts=(sigma, sigma_next), rest=rest, weights=weights)


def dpmpp2m_step_windows(state, eps_cond, eps_uncond, guidance, out_state, *, ld_eps, sigma, a, b, c1, c2, batch,
                         frames_total, h, w, window, stride, n_win, weights, ld_guidance=0):
    """``dpmpp2m_step`` of the 8-channel ``state`` (B,8,F_total,H,W) behind the eps rows of ``n_win`` overlapping frame
    windows; layouts as for ``euler_step_windows`` (``sp_dpmpp2m_step_windows_f16``)."""
    patch, rest = _windows(frames_total, h, w, window, stride, n_win, weights)
    return _tail("sp_dpmpp2m_step_windows_f16", "dpmpp2m_step_windows", {"state": state, "out_state": out_state}, channels=8, batch=batch,
                 dims=(frames_total, h, w), patch=patch, eps=(eps_cond, eps_uncond), guidance=guidance, ld_eps=ld_eps, ld_guidance=ld_guidance,
                 consts=(sigma, a, b, c1, c2), rest=rest, weights=weights)


def euler_ancestral_step(latent, eps_cond, eps_uncond, guidance, out, *, ld_eps, sigma, sigma_down, noise_scale, seeds, step,
                         b, frames_total, h, w, window=None, stride=None, n_win=None, weights=None, ld_guidance=0):
    """The Euler ancestral update of ``latent`` (B,4,F_total,H,W): the Euler step to ``sigma_down`` plus ``noise_scale * z``,
    ``z`` the normals of (``seeds[b]``, ``step``, the element) (``sp_euler_ancestral_step_f16``).  ``weights=None``: eps rows
    ``[B][F][H*W][ld_eps]``; else the window arguments of ``euler_step_windows``."""
    patch, rest = _windows(frames_total, h, w, window, stride, n_win, weights)
    return _tail("sp_euler_ancestral_step_f16", "euler_ancestral_step", {"latent": latent, "out": out}, channels=4, batch=b,
                 dims=(frames_total, h, w), patch=patch, eps=(eps_cond, eps_uncond), guidance=guidance, ld_eps=ld_eps, ld_guidance=ld_guidance,
                 consts=(sigma, sigma_down), rest=rest, weights=weights, noise=(noise_scale, seeds, step))


def dpmpp2m_sde_step(state, eps_cond, eps_uncond, guidance, out_state, *, ld_eps, sigma, a, b, c1, c2, noise_scale, seeds, step,
                     batch, frames_total, h, w, window=None, stride=None, n_win=None, weights=None, ld_guidance=0):
    """The DPM-Solver++(2M) SDE update of the 8-channel ``state`` (B,8,F_total,H,W): ``dpmpp2m_step`` with ``noise_scale * z``
    added to the sample, not to the stored estimate (``sp_dpmpp2m_sde_step_f16``); windows as for ``euler_ancestral_step``."""
    patch, rest = _windows(frames_total, h, w, window, stride, n_win, weights)
    return _tail("sp_dpmpp2m_sde_step_f16", "dpmpp2m_sde_step", {"state": state, "out_state": out_state}, channels=8, batch=batch,
                 dims=(frames_total, h, w), patch=patch, eps=(eps_cond, eps_uncond), guidance=guidance, ld_eps=ld_eps, ld_guidance=ld_guidance,
                 consts=(sigma, a, b, c1, c2), rest=rest, weights=weights, noise=(noise_scale, seeds, step))


class TileRecord:
    """A ``models.tile_plan.TilePlan`` as the kernels take it: the ``sp_tile_plan`` record and the three weight tables on the
    device, which it keeps alive.  ``space=False``: a record for the entries that take frame windows as arguments, which read
    ``wf`` alone; ``wy`` and ``wx`` are not uploaded and stay null (the tiles entries refuse such a record)."""

    def __init__(self, plan, device, space=True):
        from . import TilePlan
        self.plan = plan
        self.wf, self.wy, self.wx = (torch.from_numpy(t).to(device).contiguous() if space or i == 0 else None
                                     for i, t in enumerate((plan.wf, plan.wy, plan.wx)))
        fr, ay, ax = plan.frames, plan.y, plan.x
        self.desc = TilePlan(frames_total=fr.frames_total, window=fr.window, stride=fr.stride, n_win=fr.n_win,
                             h=ay.frames_total, w=ax.frames_total, tile_h=ay.window, tile_w=ax.window, stride_y=ay.stride,
                             stride_x=ax.stride, n_ty=ay.n_win, n_tx=ax.n_win, wf=self.wf.data_ptr(), wy=_ptr(self.wy),
                             wx=_ptr(self.wx))


def _tiles(rec):
    """``(dims, patch, lead)`` of an entry that takes its plan as a ``TileRecord``."""
    d = rec.desc
    return (d.frames_total, d.h, d.w), (d.n_win * d.n_ty * d.n_tx, d.window, d.tile_h, d.tile_w), (ctypes.byref(d),)


def euler_step_tiles(latent, eps_cond, eps_uncond, guidance, out, *, plan, ld_eps, sigma, sigma_next, b, ld_guidance=0,
                     noise_scale=0.0, seeds=None, step=0):
    """The Euler update of ``latent`` (B,4,F_total,H,W) behind the eps rows of the patches of ``plan`` (a ``TileRecord``):
    frame windows times overlapping spatial tiles, ``[n_patch][B][window][tile_h*tile_w][ld_eps]``.  ``noise_scale != 0`` is the
    Euler ancestral update (``sigma_next`` is then sigma_down) with the noise of ``seeds`` and ``step``
    (``sp_euler_step_tiles_f16``)."""
    dims, patch, lead = _tiles(plan)
    return _tail("sp_euler_step_tiles_f16", "euler_step_tiles", {"latent": latent, "out": out}, channels=4, batch=b, dims=dims, patch=patch,
                 eps=(eps_cond, eps_uncond), guidance=guidance, ld_eps=ld_eps, ld_guidance=ld_guidance,
                 consts=(sigma, sigma_next), lead=lead, noise=(noise_scale, seeds, step))


def dpmpp2m_step_tiles(state, eps_cond, eps_uncond, guidance, out_state, *, plan, ld_eps, sigma, a, b, c1, c2, batch,
                       ld_guidance=0, noise_scale=0.0, seeds=None, step=0):
    """``dpmpp2m_step`` (``noise_scale != 0``: ``dpmpp2m_sde_step``) of the 8-channel ``state`` (B,8,F_total,H,W) behind the eps
    rows of the patches of ``plan``; layouts as for ``euler_step_tiles`` (``sp_dpmpp2m_step_tiles_f16``)."""
    dims, patch, lead = _tiles(plan)
    return _tail("sp_dpmpp2m_step_tiles_f16", "dpmpp2m_step_tiles", {"state": state, "out_state": out_state}, channels=8, batch=batch, dims=dims,
                 patch=patch, eps=(eps_cond, eps_uncond), guidance=guidance, ld_eps=ld_eps, ld_guidance=ld_guidance,
                 consts=(sigma, a, b, c1, c2), lead=lead, noise=(noise_scale, seeds, step))


def randn(out, seeds, *, scale=1.0, step=0, purpose=0):
    """``out`` (B,4,F,H,W) fp16 = ``scale * z``: video ``b``'s normals of (``seeds[b]``, ``step``, ``purpose``), whatever it is
    batched with (``sp_randn_f16``; purpose 0 = the initial latent, 1 = a sampler step's noise)."""
    if _f16(out, "out").dim() != 5 or out.shape[1] != 4 or not out.is_contiguous():
        raise ValueError(f"randn: out must be a contiguous (B, 4, F, H, W) tensor; got {tuple(out.shape)}")
    b, _, f, h, w = out.shape
    _check(load().sp_randn_f16(out.data_ptr(), _seeds(seeds, b, "randn"), scale, b, f, h, w, int(step), int(purpose), _stream()),
           "sp_randn_f16")
    return out


def philox_blocks(out, seeds, *, step=0, purpose=0):
    """``out`` int32 ``[B][n_blocks][4]``: the generator's raw words (``sp_philox_blocks_u32``)."""
    if out.dtype != torch.int32 or not out.is_cuda or out.dim() != 3 or out.shape[2] != 4 or not out.is_contiguous():
        raise ValueError(f"philox_blocks: out must be a contiguous int32 [B][n_blocks][4] tensor on the HIP device; got "
                         f"{out.dtype} {tuple(out.shape)}")
    _check(load().sp_philox_blocks_u32(out.data_ptr(), _seeds(seeds, out.shape[0], "philox_blocks"), out.shape[0], out.shape[1],
                                       int(step), int(purpose), _stream()), "sp_philox_blocks_u32")
    return out


def concat_channels(a, ca, b, cb, out, rows):
    with _Timed("concat", 0.0, 2 * 2.0 * rows * (ca + cb)):
        _check(load().sp_concat_channels_f16(a.data_ptr(), ca, b.data_ptr(), cb, out.data_ptr(), rows, _stream()),
               "sp_concat_channels_f16")
    return out


def add_rowvec(x, vec32, y, rows, c):
    _check(load().sp_add_rowvec_f16(x.data_ptr(), vec32.data_ptr(), y.data_ptr(), rows, c, _stream()), "sp_add_rowvec_f16")
    return y


def dummy_unet_forward(x, w1, b1, w2, b2, ln_w, ln_b, gain, ln_eps):
    """DummyUNet forward on a HIP device (fp32, (B,C,F,H,W)); see csrc/dummy_unet.hip."""
    B, C, F, H, W = x.shape
    hidden_c = w1.shape[0]
    out = torch.empty_like(x)
    hidden = torch.empty((B, hidden_c, F, H, W), dtype=torch.float32, device=x.device)
    _check(load().sp_dummy_unet_f32(x.data_ptr(), out.data_ptr(), hidden.data_ptr(), w1.contiguous().data_ptr(),
                                    b1.data_ptr(), w2.contiguous().data_ptr(), b2.data_ptr(), _ptr(ln_w), _ptr(ln_b),
                                    float(ln_eps), int(ln_w is not None), float(gain), B, C, hidden_c, F, H, W,
                                    _stream()), "sp_dummy_unet_f32")
    return out
