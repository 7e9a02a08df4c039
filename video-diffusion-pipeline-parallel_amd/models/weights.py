"""Weight re-layout for the HIP kernels (done once at load time, on any device).

All dense weights are stored fp16 ``[N][K]`` with K contiguous, which is what the MFMA weight
operand wants (``nn.Linear.weight`` already is); convolution kernels are flattened tap-major so a
64-channel K-step never crosses a tap.
"""

from __future__ import annotations

import torch


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def pack_conv3x3(w: torch.Tensor, cin_pad: int | None = None, n_pad: int | None = None) -> torch.Tensor:
    """(Cout, Cin, 3, 3) -> (Npad, 9*Cpad) fp16 with k = (ky*3+kx)*Cpad + c."""
    cout, cin = w.shape[:2]
    cp = cin_pad or round_up(cin, 64)
    npad = n_pad or round_up(cout, 64)
    out = torch.zeros(npad, 9, cp, dtype=torch.float16, device=w.device)
    out[:cout, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, 9, cin).to(torch.float16)
    return out.reshape(npad, 9 * cp).contiguous()


def fold_conv3x3_up2x(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, 3, 3) -> (4, Cout, 2, 2, Cin) in the dtype of ``w``: the 3x3 convolution behind a nearest x2 upsample as
    four 2x2 convolutions on the source image, one per parity phase p = 2*py + px of the output pixel.  The taps of output
    row 2*sy + py read upsampled rows 2*sy + py - 1 + ky, i.e. source rows sy - 1, sy, sy for py = 0 and sy, sy, sy + 1
    for py = 1: on the window rows (sy + py - 1, sy + py) the row weights are (w[0], w[1] + w[2]) and (w[0] + w[1], w[2]);
    columns alike with px.  A padded row of the upsampled image is a padded row of the source: no special case."""
    rows = (lambda k: (k[0], k[1] + k[2]), lambda k: (k[0] + k[1], k[2]))
    wt = w.permute(2, 3, 0, 1)                                      # [ky][kx][Cout][Cin]
    out = w.new_zeros((4, 2, 2) + tuple(wt.shape[2:]))              # [p][ty][tx][Cout][Cin]
    for py in range(2):
        wy = rows[py](wt)                                           # 2 x [kx][Cout][Cin]
        for px in range(2):
            for ty in range(2):
                wx = rows[px](wy[ty])
                out[2 * py + px, ty, 0], out[2 * py + px, ty, 1] = wx[0], wx[1]
    return out.permute(0, 3, 1, 2, 4).contiguous()


def pack_conv3x3_up2x(w: torch.Tensor, cin_pad: int | None = None, n_pad: int | None = None) -> torch.Tensor:
    """(Cout, Cin, 3, 3) -> (4, Npad, 4*Cpad) fp16, phase-major, k = (2*ty + tx)*Cpad + c: the operand of
    ``sp_conv_up2x_f16`` (see :func:`fold_conv3x3_up2x`).  Folded in fp32, rounded to fp16 once."""
    cout, cin = w.shape[:2]
    cp = cin_pad or round_up(cin, 64)
    npad = n_pad or round_up(cout, 64)
    out = torch.zeros(4, npad, 4, cp, dtype=torch.float16, device=w.device)
    out[:, :cout, :, :cin] = fold_conv3x3_up2x(w.float()).reshape(4, cout, 4, cin).to(torch.float16)
    return out.reshape(4, npad, 4 * cp).contiguous()


def pack_tconv3(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, 3, 1, 1) -> (Cout, 3*Cin) fp16 with k = tap*Cin + c."""
    cout, cin = w.shape[:2]
    return w[:, :, :, 0, 0].permute(0, 2, 1).reshape(cout, 3 * cin).to(torch.float16).contiguous()


def pack_linear(w: torch.Tensor) -> torch.Tensor:
    return w.reshape(w.shape[0], -1).to(torch.float16).contiguous()


def interleave_geglu(w: torch.Tensor, b: torch.Tensor | None):
    """GEGLU projection (2*inner, K): reorder rows so value/gate alternate in blocks of 16.

    Output rows [32q, 32q+16) are value rows 16q.., rows [32q+16, 32q+32) the matching gate rows, so a
    wave's adjacent 16-row MFMA sub-tiles hold (value, gate) for the same 16 output columns and the
    GEMM epilogue forms ``value * gelu(gate)`` in registers.
    """
    two_inner = w.shape[0]
    inner = two_inner // 2
    assert inner % 16 == 0
    idx = torch.arange(inner, device=w.device).reshape(-1, 16)
    order = torch.cat([idx, idx + inner], dim=1).reshape(-1)
    wi = w[order].to(torch.float16).contiguous()
    bi = None if b is None else b[order].float().contiguous()
    return wi, bi
