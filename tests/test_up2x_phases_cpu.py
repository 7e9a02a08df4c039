"""Upsampling convolutions as four 2x2 phase convolutions, without a GPU: the weight fold, a model of the kernel's row map
and column-sum tile index, the new entry's argument validation (nothing is launched on a bad argument) and the engine's
rule for taking the phase path."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

from vdpp_amd import hip
from vdpp_amd.models import unet_hip
from vdpp_amd.models import weights as W


def phase_conv(x, wf):
    """The four folded 2x2 convolutions as include/svdpipe.h states them.  x [B][C][H][W], wf [4][Cout][2][2][Cin] ->
    [B][Cout][2H][2W]: output pixel (2*sy + py, 2*sx + px) = sum over the window (sy + py - 1 + ty, sx + px - 1 + tx)."""
    b, c, hh, ww = x.shape
    out = x.new_zeros(b, wf.shape[1], 2 * hh, 2 * ww)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            acc = 0
            for ty in range(2):
                for tx in range(2):
                    win = xp[:, :, py + ty:py + ty + hh, px + tx:px + tx + ww]       # padded index = source index + 1
                    acc = acc + torch.einsum("bchw,oc->bohw", win, wf[2 * py + px, :, ty, tx])
            out[:, :, py::2, px::2] = acc
    return out


@pytest.mark.parametrize("hh,ww", [(1, 1), (1, 5), (4, 4), (5, 7)])
@pytest.mark.parametrize("cin,cout", [(64, 128), (96, 128)])
def test_fold_is_exact_and_survives_one_fp16_rounding(hh, ww, cin, cout):
    g = torch.Generator().manual_seed(hh * 100 + ww + cin)
    x = torch.randn(2, cin, hh, ww, generator=g).half().double()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).half().double()
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    got = phase_conv(x, W.fold_conv3x3_up2x(w))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())          # fp64: summation order only
    # the pack: phase-major [4][Npad][4*Cpad], k = (2*ty + tx)*Cpad + c, zero padding, folded in fp32 and rounded once
    cp = W.round_up(cin, 64)
    pack = W.pack_conv3x3_up2x(w.float(), cp, 128)
    assert pack.dtype == torch.float16 and tuple(pack.shape) == (4, 128, 4 * cp) and pack.is_contiguous()
    p5 = pack.reshape(4, 128, 2, 2, cp)
    assert not p5[..., cin:].any() and not p5[:, cout:].any()
    assert torch.equal(p5[:, :cout, :, :, :cin], W.fold_conv3x3_up2x(w.float()).half())
    got16 = phase_conv(x, p5[:, :cout, :, :, :cin].double())
    err = float((got16 - want).norm() / want.norm())
    print(f"relative L2 after the single fp16 rounding: {err:.2e}")
    assert err <= 5e-4


def kernel_rows(n_img, hin, win, gn):
    """Model of gemm_pp_kernel<256, BN, 8192>: for every row tile of the grid (phase-major, ceil(n_img*hin*win / 256) per
    phase) the output rows it stores and, with ``gn``, the tile index of its column sums."""
    rows = n_img * hin * win
    up_tiles = (rows + 255) // 256
    t = hin * win // 256 if gn else 1
    for tile_mg in range(4 * up_tiles):
        phase, tile_m = divmod(tile_mg, up_tiles)
        py, px = phase >> 1, phase & 1
        stored = []
        for m in range(tile_m * 256, min(rows, tile_m * 256 + 256)):
            img, rem = divmod(m, hin * win)
            sy, sx = divmod(rem, win)
            stored.append((img * 2 * hin + 2 * sy + py) * 2 * win + 2 * sx + px)
        frame = tile_m // t
        yield stored, (frame * 4 + phase) * t + (tile_m - frame * t)


@pytest.mark.parametrize("n_img,hin,win", [(3, 9, 11), (2, 1, 5), (2, 5, 1), (2, 16, 16), (3, 16, 32), (28, 9, 16)])
def test_row_map_writes_every_output_row_once_and_keeps_a_frames_tiles_together(n_img, hin, win):
    gn = hin * win % 256 == 0
    tiles = list(kernel_rows(n_img, hin, win, gn))
    stored = sorted(r for rows, _ in tiles for r in rows)
    assert stored == list(range(4 * n_img * hin * win))
    if gn:
        t = hin * win // 256
        per_frame = 4 * hin * win
        assert sorted(i for _, i in tiles) == list(range(4 * n_img * t))           # every tile index once
        for rows, idx in tiles:
            frames = {r // per_frame for r in rows}
            assert frames == {idx // (4 * t)}, "a tile's sums stand among the tiles of the frame its rows belong to"


def test_bad_arguments_are_refused_by_name_and_nothing_is_launched():
    lib = hip.load()
    A, Wt, D, Z, G = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000              # never dereferenced: validation comes first
    good = dict(a=A, lda=64, cin=64, n_img=2, hin=16, win=16, w=Wt, n=320, bias=None, d=D, ldd=320, gn_part=None, zero=Z)

    def call(**kw):
        v = dict(good, **kw)
        rc = lib.sp_conv_up2x_f16(v["a"], v["lda"], v["cin"], v["n_img"], v["hin"], v["win"], v["w"], v["n"], v["bias"], v["d"],
                                  v["ldd"], v["gn_part"], v["zero"], None)
        return rc, lib.sp_last_error().decode()

    for kw, word in ((dict(a=None), "null"), (dict(w=None), "null"), (dict(d=None), "null"), (dict(zero=None), "null"),
                     (dict(d=D + 8), "aligned"), (dict(cin=96), "cin=96"), (dict(cin=0), "cin=0"), (dict(n=192), "n=192"),
                     (dict(lda=56), "lda=56"), (dict(lda=68), "lda=68"), (dict(ldd=256), "ldd=256"), (dict(ldd=324), "ldd=324"),
                     (dict(hin=0), "hin=0"), (dict(n_img=-1), "n_img=-1"), (dict(n_img=1 << 20, hin=64, win=64), "fit an int"),
                     (dict(gn_part=G, hin=8, win=8), "hin*win = 64"), (dict(gn_part=G + 4), "aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg and msg.startswith("sp_conv_up2x_f16"), (kw, rc, msg)


def test_engine_takes_the_phase_path_where_it_pays():
    eng = unet_hip.SVDUNetHIP.__new__(unet_hip.SVDUNetHIP)
    eng.upsample_phases = True
    layer = lambda n, cin, pack=True: types.SimpleNamespace(n=n, cin=cin, w_up2x=object() if pack else None)
    # the benchmark: two videos of 14 frames, 72 x 128 latent -> (phases, column sums from the epilogue)
    assert eng._upsample_plan(layer(640, 640), 28, 36, 64) == (True, True)        # source frames are whole tiles: sums stay
    assert eng._upsample_plan(layer(1280, 1280), 28, 18, 32) == (True, False)     # trades them for one statistics pass
    assert eng._upsample_plan(layer(1280, 1280), 28, 9, 16) == (True, False)      # output frames of 576 rows: never had any
    # tests/test_launch_plan_cpu.py, UNetConfig.tiny(256) at 16 x 16 and 32 x 32, tiny(64) at 16 x 24
    assert eng._upsample_plan(layer(1024, 1024), 6, 2, 2) == (True, False)
    assert eng._upsample_plan(layer(1024, 1024), 6, 4, 4) == (True, False)
    assert eng._upsample_plan(layer(512, 512), 6, 8, 8) == (False, True)          # too small to pay for the pass: nine taps
    assert eng._upsample_plan(layer(1024, 1024), 2, 8, 8) == (False, True)
    assert eng._upsample_plan(layer(512, 512), 2, 16, 16) == (True, True)
    assert eng._upsample_plan(layer(256, 256), 3, 4, 6) == (True, False)
    assert eng._upsample_plan(layer(128, 128, pack=False), 3, 8, 12) == (False, True)   # no 256- / 320-column tiles: no pack
    eng.upsample_phases = False
    assert eng._upsample_plan(layer(640, 640), 28, 36, 64) == (False, True)


def test_binding_and_keyword():
    assert hip.SIGNATURES["sp_conv_up2x_f16"][1][:3] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]
    import inspect
    from vdpp_amd.hip import ops
    assert inspect.signature(ops.gemm).parameters["up2x_phases"].default is False
