"""csrc/attention_window.hip: ``sp_attn_spatial_window_f16`` against an fp64 masked softmax written from the semantics
(8 x 8 token tiles, a window of whole tiles shifted inwards at the borders) on the same fp16 operands, and the refusals."""
import pytest
import torch

from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda"


def window_mask(h, w, wh, ww):
    """bool [h*w][h*w]: may query token (row) see key token (column)?"""
    gh, gw = h // 8, w // 8
    eh, ew = min(wh, gh), min(ww, gw)
    ty, tx = torch.arange(h) // 8, torch.arange(w) // 8                       # tile row of token row y, tile column of x
    y0, x0 = (ty - wh // 2).clamp(0, gh - eh), (tx - ww // 2).clamp(0, gw - ew)
    my = (ty[None, :] >= y0[:, None]) & (ty[None, :] < y0[:, None] + eh)      # [query y][key y]
    mx = (tx[None, :] >= x0[:, None]) & (tx[None, :] < x0[:, None] + ew)      # [query x][key x]
    return (my[:, None, :, None] & mx[None, :, None, :]).reshape(h * w, h * w)


def reference(x, mask, batch, heads, scale=0.125):
    """x: fp16 rows [batch*hw][3*heads*64] (fused QKV) -> fp64 O rows [batch*hw][heads*64]."""
    q, k, v = [t.double().view(batch, -1, heads, 64).transpose(1, 2) for t in x.chunk(3, dim=1)]
    logits = (q @ k.transpose(-1, -2) * scale).masked_fill(~mask, float("-inf"))
    return (torch.softmax(logits, -1) @ v).transpose(1, 2).reshape(x.shape[0], heads * 64)


SHAPES = [(8, 8, 1, 1),          # one tile
          (8, 40, 1, 3),         # 1 x 5 tiles: clamping at both ends in x, a strip with one live wave, waves skip different tiles
          (40, 8, 3, 1),         # clamping in y, tile-row stepping at the narrowest grid
          (24, 72, 3, 5),        # the window spans the y axis; 9 tile columns: the ragged strip and interior windows
          (16, 16, 9, 9)]        # the window is larger than the grid: full attention


@pytest.mark.parametrize("gain", [1, 3])
@pytest.mark.parametrize("h,w,wh,ww", SHAPES)
def test_attn_spatial_window_matches_fp64_masked_softmax(h, w, wh, ww, gain):
    """q, k, v are column slices of a fused QKV buffer whose pitch exceeds 3c; its slack columns and a guard row on either
    side are NaN.  Gain 3 on q and k: logits of standard deviation 9, peaked rows.  The bound is the one
    tests/test_attn_kv_gpu.py holds sp_attn_spatial_kv_f16 to against fp64 (rel-L2 3e-3, max 2e-2): the same contract."""
    from vdpp_amd.hip import ops
    batch, heads = 2, 2
    c, rows = heads * 64, batch * h * w
    pitch = 3 * c + 8
    g = torch.Generator().manual_seed(h * w + wh + ww)
    x = torch.randn(rows, 3 * c, generator=g)
    x[:, :2 * c] *= gain
    x = x.half()
    buf = torch.full((rows + 2, pitch), float("nan"), dtype=torch.float16)
    buf[1:-1, :3 * c] = x
    qkv = buf.to(DEV)[1:-1]
    o = torch.full((rows, c + 8), 5.0, dtype=torch.float16, device=DEV)
    ops.attn_spatial_window(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:3 * c], o, ldq=pitch, ldk=pitch, ldv=pitch, ldo=c + 8,
                            batch=batch, h=h, w=w, heads=heads, wh=wh, ww=ww)
    ref = reference(x, window_mask(h, w, wh, ww), batch, heads).float()
    assert bool((o[:, c:] == 5.0).all()), "pitch slack written"
    check(o[:, :c], ref, l2=3e-3, mx=2e-2)


OK = dict(q=0, ldq=384, ldo=128, h=16, w=16, wh=3, ww=3)
REFUSED = [dict(wh=2), dict(ww=0), dict(h=12), dict(w=20), dict(ldo=120), dict(q=8)]


@pytest.mark.parametrize("bad", REFUSED, ids=["-".join(f"{k}={v}" for k, v in b.items()) for b in REFUSED])
def test_refusals_raise_and_leave_the_output_untouched(bad):
    from vdpp_amd.hip import ops
    a = dict(OK, **bad)
    qkv = torch.ones(2 * 256 + 1, 384, dtype=torch.float16, device=DEV)
    o = torch.full((2 * 256, 128), 5.0, dtype=torch.float16, device=DEV)
    q = qkv.view(-1)[a["q"] // 2:][:2 * 256 * 384].view(-1, 384)[:, :128]      # (q = 8: eight bytes into the buffer, misaligned)
    with pytest.raises(ops.HipKernelError, match="sp_attn_spatial_window_f16"):
        ops.attn_spatial_window(q, qkv[:, 128:256], qkv[:, 256:], o, ldq=a["ldq"], ldk=384, ldv=384, ldo=a["ldo"], batch=2,
                                h=a["h"], w=a["w"], heads=2, wh=a["wh"], ww=a["ww"])
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())
