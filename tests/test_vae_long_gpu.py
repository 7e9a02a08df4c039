"""VAE mid-block attention beyond 16,384 tokens per frame: the streaming row softmax
(``sp_softmax_rows_long_f32``) against the register kernel byte for byte and against fp64 above its limit, the row-blocked
attention of ``_VAEKernels._run_attn`` against the short route and an fp64 evaluation, both engines on the long route at
small and at above-limit sizes, a decoder call whose activations pass 2^32 bytes, and ``modes.generate`` end to end."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _ops():
    from vdpp_amd.hip import ops
    return ops


def _logits(rows, cols, ld=None):
    """The inputs of tests/test_vae_gpu.py::test_softmax_rows_f32: huge logits, logits near 60,000, one dominant logit."""
    g = torch.Generator().manual_seed(rows * cols)
    x = torch.randn(rows, ld or cols, generator=g) * 50.0
    x[0] = x[0] * 6000.0                                     # |logit| up to ~1e6
    x[1] = 60000.0 + torch.randn(ld or cols, generator=g) * 3.0
    if rows > 2:
        x[2, 5] = 2.0e5                                      # one dominant logit beyond fp16's largest number
    return x


SCALE = 0.37


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("rows,cols", [(5, 256), (9, 2304), (4, 9216), (3, 16384)])
def test_long_softmax_returns_the_register_kernels_bytes(rows, cols, inplace):
    """Up to 16,384 columns the streaming kernel keeps the register kernel's assignment of elements to threads and its order
    of accumulation and reduction: the same bytes, in place and out of place, with no tolerance."""
    ops = _ops()
    x = _logits(rows, cols)
    if inplace:
        a, b = x.to(DEV), x.to(DEV)
        ops.softmax_rows_f32(a, a.view(torch.float16), rows=rows, cols=cols, scale=SCALE, ld=cols, ldo=2 * cols)
        ops.softmax_rows_long_f32(b, b.view(torch.float16), rows=rows, cols=cols, scale=SCALE, ld=cols, ldo=2 * cols)
        short, long_ = a.view(torch.float16)[:, :cols], b.view(torch.float16)[:, :cols]
        assert torch.equal(a.view(torch.int32)[:, cols // 2:], b.view(torch.int32)[:, cols // 2:])   # the rows' untouched backs
    else:
        xd = x.to(DEV)
        short = torch.full((rows, cols + 8), 3.0, dtype=torch.float16, device=DEV)
        long_ = torch.full((rows, cols + 8), 3.0, dtype=torch.float16, device=DEV)
        ops.softmax_rows_f32(xd, short, rows=rows, cols=cols, scale=SCALE)
        ops.softmax_rows_long_f32(xd, long_, rows=rows, cols=cols, scale=SCALE)
        assert float((long_[:, cols:].float() - 3.0).abs().max()) == 0.0 and torch.equal(xd.cpu(), x)
    assert torch.isfinite(long_.float()).all() and float(long_[2, 5]) == 1.0
    assert torch.equal(short.contiguous().view(torch.int16), long_.contiguous().view(torch.int16))


@pytest.mark.parametrize("rows,cols,ld,ldo", [(5, 256, 260, 272), (4, 2304, 2560, 2312), (3, 9216, 9220, 9224),
                                              (3, 16384, 16392, 16400), (3, 20736, 20740, 20744)])
def test_long_softmax_with_row_pitches(rows, cols, ld, ldo):
    """ld > cols, out of place: the columns behind ``cols`` of ``out`` stay, ``x`` is unchanged, and (where the register kernel
    takes the length) the bytes are the register kernel's."""
    ops = _ops()
    x = _logits(rows, cols, ld)
    xd = x.to(DEV)
    out = torch.full((rows, ldo), 3.0, dtype=torch.float16, device=DEV)
    ops.softmax_rows_long_f32(xd, out, rows=rows, cols=cols, scale=SCALE, ld=ld, ldo=ldo)
    assert float((out[:, cols:].float() - 3.0).abs().max()) == 0.0 and torch.equal(xd.cpu(), x)
    got = out[:, :cols].float().cpu()
    want = torch.softmax(x[:, :cols].double() * SCALE, dim=-1).float()
    assert float((got - want).abs().max()) <= 1e-3 and rel_l2(got, want) <= 2e-3
    if cols <= 16384:
        ref = torch.full((rows, ldo), 3.0, dtype=torch.float16, device=DEV)
        ops.softmax_rows_f32(xd, ref, rows=rows, cols=cols, scale=SCALE, ld=ld, ldo=ldo)
        assert torch.equal(ref.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("rows,cols", [(3, 16388), (3, 20736), (2, 36864)])
def test_long_softmax_above_the_register_limit(rows, cols, inplace):
    """16,388 is the first length ``sp_softmax_rows_f32`` refuses and no multiple of the 1,024-logit chunk; 20,736 and 36,864
    are the frames of 864 x 1536 and 1152 x 2048 pixels.  Against torch.softmax in fp64 at the bounds of
    ``test_softmax_rows_f32`` (max abs 1e-3, rel-L2 2e-3); a dominant logit gives exactly 1.0 and a NaN row stays NaN."""
    ops = _ops()
    with pytest.raises(ops.HipKernelError, match="<= 16384"):
        ops.softmax_rows_f32(torch.zeros(1, cols, device=DEV), torch.zeros(1, cols, dtype=torch.float16, device=DEV), rows=1,
                             cols=cols)

    def run(x):
        xd = x.to(DEV)
        if inplace:
            out = xd.view(torch.float16)
            ops.softmax_rows_long_f32(xd, out, rows=x.shape[0], cols=cols, scale=SCALE, ld=cols, ldo=2 * cols)
            return out[:, :cols].float().cpu()
        out = torch.full((x.shape[0], cols + 8), 3.0, dtype=torch.float16, device=DEV)
        ops.softmax_rows_long_f32(xd, out, rows=x.shape[0], cols=cols, scale=SCALE)
        assert float((out[:, cols:].float() - 3.0).abs().max()) == 0.0
        assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))              # (bits: a NaN equals itself)
        return out[:, :cols].float().cpu()

    x = _logits(rows, cols)
    got = run(x)
    want = torch.softmax(x.double() * SCALE, dim=-1).float()
    err_abs, err_rel = float((got - want).abs().max()), rel_l2(got, want)
    print(f"long softmax {rows} x {cols} {'in place' if inplace else 'out of place'}: max abs {err_abs:.2e}, rel-L2 {err_rel:.2e}")
    assert torch.isfinite(got).all()
    assert err_abs <= 1e-3 and err_rel <= 2e-3
    assert float((got.sum(-1) - 1).abs().max()) <= 4e-3

    # a dominant logit far from the front, in the last (partial) chunk, and a NaN between two finite rows
    y = torch.randn(4, cols, generator=torch.Generator().manual_seed(cols)) * 50.0
    y[0, cols - 3] = 2.0e5
    y[1, 16385] = 2.0e5
    y[2, cols - 2] = float("nan")
    got = run(y)
    assert float(got[0, cols - 3]) == 1.0 and float(got[0].sum()) == 1.0
    assert float(got[1, 16385]) == 1.0 and float(got[1].sum()) == 1.0
    assert torch.isnan(got[2]).any() and torch.isfinite(got[3]).all() and torch.isfinite(got[:2]).all()
    assert rel_l2(got[3], torch.softmax(y[3].double() * SCALE, -1).float()) <= 2e-3


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("cols", [16388, 20736, 36864])
def test_long_softmax_exact_patterns_above_the_limit(cols, inplace):
    """No tolerance: logits 0 on 2^k selected columns and -1e30 elsewhere give 2^-k there and 0 elsewhere, bit for bit (the sum
    is an integer below 2^24, so every order of summation gives the same bytes).  The selected columns include column 0, the
    last column and both sides of 16,384.  A column that is lost, counted twice or stored in the wrong place changes bytes."""
    ops = _ops()
    g = torch.Generator().manual_seed(cols)
    must = [0, cols - 1, 16383, 16384]
    sel = [[c] for c in must]                                         # k = 0: one row per interesting column
    for k in (5, 12):
        rest = [c for c in torch.randperm(cols, generator=g).tolist() if c not in must][: 2 ** k - len(must)]
        sel.append(must + rest)
    ks = [0, 0, 0, 0, 5, 12]
    x = torch.full((len(sel), cols), -1.0e30)
    want = torch.zeros(len(sel), cols)
    for r, (cs, k) in enumerate(zip(sel, ks)):
        assert len(set(cs)) == 2 ** k
        x[r, cs] = 0.0
        want[r, cs] = 2.0 ** -k
    xd = x.to(DEV)
    if inplace:
        out = xd.view(torch.float16)
        ops.softmax_rows_long_f32(xd, out, rows=len(sel), cols=cols, ld=cols, ldo=2 * cols)
    else:
        out = torch.empty((len(sel), cols), dtype=torch.float16, device=DEV)
        ops.softmax_rows_long_f32(xd, out, rows=len(sel), cols=cols)
    got = out[:, :cols].cpu()
    assert torch.equal(got.contiguous().view(torch.int16), want.half().view(torch.int16))


def test_long_softmax_refusals():
    import ctypes

    from vdpp_amd import hip
    ops = _ops()
    x = torch.zeros(4, 20744, device=DEV)
    out = torch.zeros(4, 20744, dtype=torch.float16, device=DEV)
    with pytest.raises(ops.HipKernelError, match="cols a multiple of 4"):
        ops.softmax_rows_long_f32(x, out, rows=4, cols=20738)
    with pytest.raises(ops.HipKernelError, match="ld=20736"):
        ops.softmax_rows_long_f32(x, out, rows=4, cols=20740, ld=20736)
    with pytest.raises(ops.HipKernelError, match="ldo=20736"):
        ops.softmax_rows_long_f32(x, out, rows=4, cols=20740, ldo=20736)
    with pytest.raises(ops.HipKernelError, match="in place needs ldo == 2 \\* ld"):
        ops.softmax_rows_long_f32(x, x.view(torch.float16), rows=4, cols=20736, ld=20744, ldo=20744)
    with pytest.raises(ops.HipKernelError, match="<= 16777216"):
        ops.softmax_rows_long_f32(x, out, rows=1, cols=(1 << 24) + 4, ld=1 << 25, ldo=1 << 25)
    with pytest.raises(TypeError):
        ops.softmax_rows_long_f32(x.half(), out, rows=4, cols=20736)
    lib = hip.load()
    assert lib.sp_softmax_rows_long_f32(None, 256, out.data_ptr(), 256, 1, 256, 1.0, None) == -1
    assert b"sp_softmax_rows_long_f32: null pointer" in lib.sp_last_error()
    assert lib.sp_softmax_rows_long_f32(x.data_ptr(), 256, None, 256, 1, 256, 1.0, None) == -1
    assert b"sp_softmax_rows_long_f32: null pointer" in lib.sp_last_error()
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0 and float(out.abs().max()) == 0.0          # nothing was launched


# ------------------------------------------------------------------------------------------------ the attention block
def _decoder(seed=5, qk_gain=1.0):
    """Tiny decoder whose mid-block attention has its q / k projections scaled by ``qk_gain``: 4 makes the softmax peaked (logits
    of +-25 or so), so that a query row's output is its own and a block that reads other rows' queries is an O(1) error; 300
    takes the logits beyond fp16's 65,504 (tests/test_vae_gpu.py::test_mid_block_attention_with_logits_beyond_fp16)."""
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    cfg = VAEDecoderConfig.tiny(64)
    dec = TemporalDecoderHIP(cfg, random_state_dict(cfg, seed=seed), DEV)
    p = dec.mid[1]
    for name in ("q", "k"):
        p[name].w = (p[name].w.float() * qk_gain).half()
        p[name].bias = p[name].bias * qk_gain
    return cfg, dec, p


def _attn_ref(cfg, p, x, n_img, hw, rows=None):
    """fp64 evaluation of the block on the engine's fp16-rounded weights, as test_mid_block_attention_with_logits_beyond_fp16
    writes it out; ``rows``: only these query rows of every image (a row's output depends on no other query row)."""
    c = p["c"]
    xn = F.group_norm(x.double().reshape(n_img, hw, c).permute(0, 2, 1), cfg.norm_groups, p["norm"].g.double().cpu(),
                      p["norm"].b.double().cpu(), eps=p["norm"].eps).permute(0, 2, 1)
    xn = xn.half().double()                                                   # the engine stores the normalised rows in fp16
    k = (xn @ p["k"].w.double().cpu().t() + p["k"].bias.double().cpu()).half().double()
    v = xn @ p["wv"].double().cpu().t() + p["bv"].double().cpu()
    xq, xr = (xn, x.double().reshape(n_img, hw, c)) if rows is None else (xn[:, rows], x.double().reshape(n_img, hw, c)[:, rows])
    q = (xq @ p["q"].w.double().cpu().t() + p["q"].bias.double().cpu()).half().double()
    logits = q @ k.transpose(1, 2) / (c ** 0.5)
    o = torch.softmax(logits, dim=-1) @ v
    want = o.half().double() @ p["out"].w.double().cpu().t() + p["out"].bias.double().cpu() + xr
    return want.reshape(-1, c).float(), float(logits.abs().max())


def _run(dec, p, x, n_img, hw, *, long_from=None, cap=None):
    from vdpp_amd.models.common import _Act
    from vdpp_amd.models.vae_hip import ATTN_LONG_FROM, ATTN_SCRATCH_ELEMS
    dec.attn_long_from = ATTN_LONG_FROM if long_from is None else long_from
    dec.attn_scratch_elems = ATTN_SCRATCH_ELEMS if cap is None else cap
    try:
        return dec._run_attn(p, _Act(x.to(DEV)), n_img, hw).t.float().cpu()
    finally:
        dec.attn_long_from, dec.attn_scratch_elems = ATTN_LONG_FROM, ATTN_SCRATCH_ELEMS


@pytest.mark.parametrize("hw", [256, 768])
@pytest.mark.parametrize("qk_gain", [4.0, 300.0])
def test_row_blocked_attention_small_shapes(hw, qk_gain, monkeypatch):
    """The long route forced at 256 / 768 tokens (``attn_long_from = 0``), two images.  One block ([hw][hw] scratch): the calls
    of the short fp32 route on the same operands, so the same bytes.  R = 256 (three blocks at 768): within 2e-2 rel-L2 of the
    fp64 evaluation.  Against the short route no bound can be derived -- the contractions may take another kernel at m = 256
    than at m = hw -- so the project's figure for two kernel routes agreeing, 5e-3, is asserted and the value printed
    (profiles/vae_long_parity.txt).  Rows are distinct and the softmax is peaked (or, at gain 300, one-hot with logits beyond
    65,504), so "every block reads and writes block 0's rows" and "the last block is not written" are O(1) errors: both are
    shown once, by a monkeypatched block list, to fail the fp64 check by more than twice its bound."""
    from vdpp_amd.models import vae_hip
    cfg, dec, p = _decoder(qk_gain=qk_gain)
    c, n_img = p["c"], 2
    x = torch.randn(n_img * hw, c, generator=torch.Generator().manual_seed(9 + hw)).half()
    want, top = _attn_ref(cfg, p, x, n_img, hw)
    assert top > (1e5 if qk_gain == 300.0 else 10.0)
    short = _run(dec, p, x, n_img, hw)
    one = _run(dec, p, x, n_img, hw, long_from=0, cap=hw * hw)
    assert vae_hip.attn_row_blocks(hw, hw * hw)[1] == [(0, hw)]
    assert torch.equal(one, short), "one block must be the short route's calls"
    blocked = _run(dec, p, x, n_img, hw, long_from=0, cap=256 * hw)
    assert len(vae_hip.attn_row_blocks(hw, 256 * hw)[1]) == hw // 256
    e_ref, e_short, e_short_ref = rel_l2(blocked, want), rel_l2(blocked, short), rel_l2(short, want)
    print(f"row-blocked attention hw={hw} gain={qk_gain:g} (logits to {top:.3g}): blocks of 256 vs fp64 {e_ref:.2e}, "
          f"vs the short route {e_short:.2e}; short route vs fp64 {e_short_ref:.2e}")
    assert torch.isfinite(blocked).all() and e_ref <= 2e-2
    assert e_short <= 5e-3
    if hw == 768 and qk_gain == 4.0:
        monkeypatch.setattr(dec, "_buf", lambda rows, ch: torch.zeros((rows, ch), dtype=torch.float16, device=DEV))
        for what, blocks in (("every block is block 0", [(0, 256)] * 3), ("the last block is missing", [(0, 256), (256, 512)])):
            monkeypatch.setattr(vae_hip, "attn_row_blocks", lambda hw_, cap, blocks=blocks: (256, blocks))
            bad = rel_l2(_run(dec, p, x, n_img, hw, long_from=0, cap=256 * hw), want)
            print(f"  mutant, {what}: {bad:.2e} vs fp64")
            assert bad > 2 * 2e-2, what


def test_row_blocked_attention_natural_routing_above_the_limit():
    """16,640 tokens (65 x 256, a 130 x 128 latent), one image, default threshold and cap: four blocks (4,864 rows, the last
    2,048).  The fp64 evaluation covers 512 query rows -- the first and last row of every block and rows spread between -- which
    is exact for those rows; 2e-2 rel-L2 on them, every output finite."""
    from vdpp_amd.models import vae_hip
    cfg, dec, p = _decoder(qk_gain=4.0)
    c, hw = p["c"], 16640
    r, blocks = vae_hip.attn_row_blocks(hw)
    assert len(blocks) == 4 and dec.attn_long_from == 16384 and dec.attn_scratch_elems == 9216 * 9216
    x = torch.randn(hw, c, generator=torch.Generator().manual_seed(3)).half()
    got = _run(dec, p, x, 1, hw)
    assert torch.isfinite(got).all()
    rows = sorted({r0 for r0, _ in blocks} | {r1 - 1 for _, r1 in blocks} | set(range(7, hw, 33)[:504]))
    assert len(rows) == 512
    want, top = _attn_ref(cfg, p, x, 1, hw, rows=torch.tensor(rows))
    err = rel_l2(got[rows], want)
    print(f"row-blocked attention hw={hw}, {len(blocks)} blocks of {r} (logits to {top:.3g}): {err:.2e} vs fp64 on {len(rows)} rows")
    assert err <= 2e-2


def test_token_counts_above_the_limit_must_be_multiples_of_256():
    from vdpp_amd.models.common import _Act
    cfg, dec, p = _decoder()
    hw = 16448                                                     # 257 x 64
    with pytest.raises(ValueError, match=r"16448 tokens.*above 16,384 cells need \(H/8\)\*\(W/8\) to be a multiple of 256"):
        dec._run_attn(p, _Act(torch.zeros(hw, p["c"], dtype=torch.float16, device=DEV)), 1, hw)
    with pytest.raises(ValueError, match="multiple of 256"):
        dec.decode_latents_uint8(torch.zeros(1, 4, 1, 257, 64, dtype=torch.float16, device=DEV), 1)


# ------------------------------------------------------------------------------------------------ the engines
def _pair(cfg_name, seed):
    from oracle.vae_temporal_decoder_ref import TemporalDecoderRef
    from oracle.vae_temporal_decoder_ref import VAEDecoderConfig as RefCfg
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    cfg = VAEDecoderConfig.tiny(64) if cfg_name == "tiny" else VAEDecoderConfig.svd()
    rcfg = RefCfg.tiny(64) if cfg_name == "tiny" else RefCfg.svd()
    sd = random_state_dict(cfg, seed=seed)
    hip = TemporalDecoderHIP(cfg, sd, DEV)
    ref = TemporalDecoderRef(rcfg).eval()
    ref.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return hip, ref


def test_decoder_on_the_long_route_matches_oracle_and_default_route():
    """Whole decoder, 3 frames of a 16 x 16 latent (256 tokens), with every frame sent to the long route: 2e-2 rel-L2 against the
    oracle, and the default route's bytes (one block: the same calls)."""
    hip, ref = _pair("tiny", 5)
    z = torch.randn(3, 4, 16, 16, generator=torch.Generator().manual_seed(11)).half()
    base = hip.decode(z.to(DEV), 3)
    hip.attn_long_from = 0
    got = hip.decode(z.to(DEV), 3)
    torch.cuda.synchronize()
    with torch.no_grad():
        want = ref(z.float(), 3)
    assert got.shape == (3, 3, 128, 128) and torch.isfinite(got).all()
    assert rel_l2(got.float().cpu(), want) <= 2e-2
    assert torch.equal(got, base)


def test_encoder_on_the_long_route_matches_oracle_and_default_route():
    from oracle.vae_temporal_decoder_ref import EncoderRef, encode_image_latents
    from oracle.vae_temporal_decoder_ref import VAEDecoderConfig as RefCfg
    from vdpp_amd.models.vae_hip import ImageEncoderHIP, VAEDecoderConfig, random_encoder_state_dict
    cfg = VAEDecoderConfig.tiny(64)
    sd = random_encoder_state_dict(cfg, seed=7)
    hip = ImageEncoderHIP(cfg, sd, DEV)
    ref = EncoderRef(RefCfg.tiny(64)).eval()
    ref.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    img = torch.randn(1, 3, 128, 128, generator=torch.Generator().manual_seed(13)).clamp(-1.5, 1.5).half()
    base = hip.encode_image_latents(img.to(DEV), 3)
    hip.attn_long_from = 0
    got = hip.encode_image_latents(img.to(DEV), 3)
    torch.cuda.synchronize()
    want = encode_image_latents(img.float(), ref, 3)
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert rel_l2(got.float().cpu(), want) <= 2e-2
    assert torch.equal(got, base)


def test_long_route_knob_from_the_environment(monkeypatch):
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    cfg = VAEDecoderConfig.tiny(64)
    sd = random_state_dict(cfg, seed=1)
    assert TemporalDecoderHIP(cfg, sd, DEV).attn_long_from == 16384
    monkeypatch.setenv("VDPP_VAE_LONG_ATTN_FROM", "0")
    assert TemporalDecoderHIP(cfg, sd, DEV).attn_long_from == 0


def test_engines_above_the_limit():
    """A 130 x 128 latent (16,640 tokens, 1040 x 1024 pixels): both engines refused this size before the long route."""
    from vdpp_amd.models.vae_hip import (ImageEncoderHIP, TemporalDecoderHIP, VAEDecoderConfig, random_encoder_state_dict,
                                         random_state_dict)
    cfg = VAEDecoderConfig.tiny(64)
    dec = TemporalDecoderHIP(cfg, random_state_dict(cfg, seed=5), DEV)
    g = torch.Generator().manual_seed(17)
    lat = (torch.randn(1, 4, 2, 130, 128, generator=g) * 0.18215).half().to(DEV)
    frames = dec.decode_latents_uint8(lat, 2)
    assert frames.shape == (1, 2, 1040, 1024, 3) and frames.dtype == torch.uint8
    f = frames.float()
    assert float(f.std()) > 1.0 and float(f[0, 0, -8:].std()) > 1.0 and not torch.equal(frames[0, 0], frames[0, 1])
    assert torch.equal(frames, dec.decode_latents_uint8(lat, 2)), "two decodes of the same latent differ"
    enc = ImageEncoderHIP(cfg, random_encoder_state_dict(cfg, seed=7), DEV)
    img = torch.randn(1, 3, 1040, 1024, generator=g).clamp(-1.5, 1.5).half().to(DEV)
    out = enc.encode_image_latents(img, 2)
    assert out.shape == (1, 4, 2, 130, 128) and torch.isfinite(out).all() and float(out.float().std()) > 1e-3


def test_decoder_beyond_4_gib_two_kernel_routes_agree_and_are_deterministic():
    """The property of tests/test_vae_gpu.py's full-size test at 864 x 1536 pixels, 14 frames, the real widths: 18.6 M rows per
    activation at the last level, 4.76 GB tensors whose byte offsets pass 2^32, 20,736 tokens per frame in the mid block (six
    query-row blocks).  Two decodes are bit-identical, the decode through the small-tile kernels agrees within that test's 5e-3,
    the last rows of the last frame carry signal and the last two frames differ."""
    from vdpp_amd.hip import ops
    hip, _ = _pair("svd", 3)
    z = (torch.randn(14, 4, 108, 192, generator=torch.Generator().manual_seed(31)) * 4.0).half().to(DEV)
    a = hip.decode(z, 14)
    b = hip.decode(z, 14)
    torch.cuda.synchronize()
    assert a.shape == (14, 3, 864, 1536) and torch.isfinite(a).all()
    assert torch.equal(a, b), "two decodes of the same latent differ"
    del b
    with ops.gemm_route(1):                          # small tiles only: neither gemm_pp.hip nor gemm_ps.hip
        c = hip.decode(z, 14)
    torch.cuda.synchronize()
    err = float((c.float() - a.float()).double().norm() / a.float().double().norm())
    print(f"decode at 864 x 1536 x 14: kernel routes agree to rel-L2 {err:.2e}")
    assert err <= 5e-3, f"kernel routes disagree beyond 2^32 bytes: rel_l2={err:.3e}"
    assert float(a[-1, :, -8:, :].float().abs().mean()) > 1e-3 and not torch.equal(a[-1], a[-2])
    assert float(a[:, :, 432, :].float().abs().mean()) > 1e-3          # (rows in the middle of every frame as well)


def test_decoder_refuses_a_call_of_more_rows_than_an_int_and_names_the_chunk_that_fits():
    """What is 32 bits wide in a decoder call is the row index of the contractions: a call of 2^31 rows at the last level is
    refused before anything is launched, with the largest ``decode_chunk_size`` that fits."""
    hip, _ = _pair("tiny", 1)
    lat = torch.zeros(1, 4, 2, 4096, 4096, dtype=torch.float16, device=DEV)      # 2 x 64 x 2^24 = 2^31 rows
    with pytest.raises(ValueError, match="largest decode_chunk_size that fits is 1$"):
        hip.decode_latents_uint8(lat, 2)
    with pytest.raises(ValueError, match="largest decode_chunk_size that fits is 1$"):
        hip.decode_latents(lat, 2, decode_chunk_size=2)


# ------------------------------------------------------------------------------------------------ end to end
def test_generate_mode_above_the_limit(monkeypatch, tmp_path):
    """``modes.generate --tiny --random-init`` at 1040 x 1024 pixels (16,640 cells: two tiles of 640 x 1024, 400 apart), 2 steps,
    2 frames: image encode, tiled denoising and decode all at the large size; the ``.npy`` holds frames of the total size."""
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.modes import generate
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    src = tmp_path / "in.png"
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (130, 128, 3), dtype=np.uint8)).save(src)
    out = tmp_path / "out.npy"
    generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_long", "--log-level", "WARNING",
                   "--random-init", "--tiny", "--input-image", str(src), "--height", "1040", "--width", "1024",
                   "--tile-height", "640", "--tile-width", "1024", "--tile-stride-y", "400", "--tile-stride-x", "1024",
                   "--num-frames", "2", "--total-steps", "2", "--output", str(out)])
    assert not torch.distributed.is_initialized()
    frames = np.load(out)
    assert frames.shape[-4:] == (2, 1040, 1024, 3) and frames.dtype == np.uint8
    assert int(frames.max()) > int(frames.min())
