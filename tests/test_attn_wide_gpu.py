"""Fused single-head attention with a wide head (``sp_attn_wide_f16``): the kernel against fp64 at
every head width and at ragged token counts, late maxima and logits beyond fp16, the VAE engines on ``attention="fused"``
against an fp64 evaluation of the block and against the composed route, refusals, and ``modes.generate`` end to end."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 2                                   # guard rows in front of and behind every buffer


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _wide(q, k, v, *, batch, seq, d, scale, bias=None):
    """Runs the kernel on q, k, v [batch*seq][d] (fp16, CPU) laid out as columns of one pitched buffer between NaN guard
    rows, with a pitched output between sentinel rows; returns the output rows (CPU, fp16) after checking the sentinels."""
    from vdpp_amd.hip import ops
    rows, ld, ldo = batch * seq, 3 * d + 8, d + 16
    buf = torch.full((rows + 2 * GUARD, ld), float("nan"), dtype=torch.float16)
    buf[GUARD:-GUARD, :d], buf[GUARD:-GUARD, d:2 * d], buf[GUARD:-GUARD, 2 * d:3 * d] = q, k, v
    buf, out = buf.to(DEV), torch.full((rows + 2 * GUARD, ldo), 7.0, dtype=torch.float16, device=DEV)
    body = buf[GUARD:-GUARD]
    ops.attn_wide(body[:, :d], body[:, d:2 * d], body[:, 2 * d:], out[GUARD:-GUARD], ldq=ld, ldk=ld, ldv=ld, ldo=ldo, batch=batch,
                  seq=seq, head_dim=d, scale=scale, bias=None if bias is None else bias.to(DEV))
    out = out.cpu()
    assert bool((out[:GUARD] == 7.0).all() and (out[-GUARD:] == 7.0).all() and (out[:, d:] == 7.0).all()), "wrote outside o"
    return out[GUARD:-GUARD, :d]


def _ref(q, k, v, batch, seq, scale, bias=None):
    q, k, v = (t.double().reshape(batch, seq, -1) for t in (q, k, v))
    o = torch.softmax(q @ k.transpose(1, 2) * scale, dim=-1) @ v
    return (o if bias is None else o + bias.double()).reshape(batch * seq, -1)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("batch,seq", [(1, 40), (2, 64), (2, 129), (1, 333)])
@pytest.mark.parametrize("d", [128, 256, 512])
def test_kernel_parity(d, batch, seq, with_bias):
    """Less than one key tile, exactly one, one row past a query block, several tiles ragged on both sides; the bound of
    tests/test_kernels_gpu.py::test_attention_spatial (Gaussian q, k at scale 1/sqrt(d): the same logit statistics)."""
    g = torch.Generator().manual_seed(1000 * d + seq)
    q, k, v = (torch.randn(batch * seq, d, generator=g).half() for _ in range(3))
    bias = torch.randn(d, generator=g) if with_bias else None
    got = _wide(q, k, v, batch=batch, seq=seq, d=d, scale=1 / math.sqrt(d), bias=bias)
    want = _ref(q, k, v, batch, seq, 1 / math.sqrt(d), bias)
    err_rel, err_abs = rel_l2(got, want), float((got.double() - want).abs().max())
    print(f"attn_wide d={d} batch={batch} seq={seq} bias={with_bias}: rel-L2 {err_rel:.2e}, max abs {err_abs:.2e}")
    assert err_rel <= 3e-3 and err_abs <= 2e-2


def test_late_maximum_rescales_the_accumulator():
    """Three keys far down the row dominate chosen queries (as test_attention_spatial_online_softmax_rescale plants them): the
    256-register accumulator is rescaled late, in a ragged last tile as well."""
    d, seq = 512, 333
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(seq, d, generator=g).half() for _ in range(3))
    for key, query in ((200, 5), (290, 130), (332, 331)):
        k[key] = (q[query].float() * 3.0).half()
    got = _wide(q, k, v, batch=1, seq=seq, d=d, scale=1 / math.sqrt(d))
    want = _ref(q, k, v, 1, seq, 1 / math.sqrt(d))
    assert rel_l2(got, want) <= 3e-3 and float((got.double() - want).abs().max()) <= 2e-2
    assert rel_l2(got[5], v[200]) <= 1e-2                    # (the planted key took the row)


def test_logits_beyond_fp16_give_a_one_hot_softmax_bit_for_bit():
    d, seq = 512, 333
    g = torch.Generator().manual_seed(11)
    q = (64.0 * torch.randn(seq, d, generator=g)).half()
    v = torch.randn(seq, d, generator=g).half()
    p = torch.softmax(q.double() @ q.double().t() / math.sqrt(d), dim=-1)
    assert float((q.double() @ q.double().t()).diagonal().min() / math.sqrt(d)) > 65504.0
    assert float((p.sum(-1) - p.diagonal()).max()) < 2.0 ** -24, "the seed's softmax is not one-hot in fp32"
    got = _wide(q, q, v, batch=1, seq=seq, d=d, scale=1 / math.sqrt(d))
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got.contiguous().view(torch.int16), v.view(torch.int16))


# ------------------------------------------------------------------------------------------------ the engine
def _decoder(attention, qk_gain=4.0, seed=5):
    """tests/test_vae_long_gpu.py's tiny decoder with peaked mid-block attention (q / k projections scaled by ``qk_gain``)."""
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    cfg = VAEDecoderConfig.tiny(64)
    dec = TemporalDecoderHIP(cfg, random_state_dict(cfg, seed=seed), DEV, attention=attention)
    p = dec.mid[1]
    for name in ("q", "k"):
        p[name].w = (p[name].w.float() * qk_gain).half()
        p[name].bias = p[name].bias * qk_gain
    return cfg, dec, p


def _block_ref(cfg, p, x, n_img, hw, rows=None):
    """fp64 evaluation of the whole block (norm, projections, attention, output projection, residual) on the engine's
    fp16-rounded weights; ``rows``: only these query rows of every image."""
    c = p["c"]
    xr = x.double().reshape(n_img, hw, c)
    xn = F.group_norm(xr.permute(0, 2, 1), cfg.norm_groups, p["norm"].g.double().cpu(), p["norm"].b.double().cpu(),
                      eps=p["norm"].eps).permute(0, 2, 1).half().double()
    k = (xn @ p["k"].w.double().cpu().t() + p["k"].bias.double().cpu()).half().double()
    v = xn @ p["wv"].double().cpu().t() + p["bv"].double().cpu()
    if rows is not None:
        xn, xr = xn[:, rows], xr[:, rows]
    q = (xn @ p["q"].w.double().cpu().t() + p["q"].bias.double().cpu()).half().double()
    o = torch.softmax(q @ k.transpose(1, 2) / c ** 0.5, dim=-1) @ v
    return (o.half().double() @ p["out"].w.double().cpu().t() + p["out"].bias.double().cpu() + xr).reshape(-1, c).float()


def _run(dec, p, x, n_img, hw):
    from vdpp_amd.models.common import _Act
    return dec._run_attn(p, _Act(x.to(DEV)), n_img, hw).t.float().cpu()


@pytest.mark.parametrize("hw", [256, 768])
def test_engine_fused_against_fp64_and_the_composed_route(hw):
    cfg, fused, p = _decoder("fused")
    _, composed, pc = _decoder("composed")
    assert fused.attention == "fused" and composed.attention == "composed" and p["c"] == 256
    x = torch.randn(2 * hw, p["c"], generator=torch.Generator().manual_seed(9 + hw)).half()
    got, base, want = _run(fused, p, x, 2, hw), _run(composed, pc, x, 2, hw), _block_ref(cfg, p, x, 2, hw)
    print(f"fused mid-block attention hw={hw}: vs fp64 {rel_l2(got, want):.2e}, vs composed {rel_l2(got, base):.2e}")
    assert torch.isfinite(got).all() and rel_l2(got, want) <= 2e-2
    assert rel_l2(got, base) <= 5e-3


def test_engine_fused_takes_the_token_count_the_composed_route_refuses():
    from vdpp_amd.models.common import _Act
    hw = 16448                                                     # 257 x 64
    cfg, composed, pc = _decoder("composed")
    x = torch.randn(hw, pc["c"], generator=torch.Generator().manual_seed(3)).half()
    with pytest.raises(ValueError, match="multiple of 256"):
        composed._run_attn(pc, _Act(x.to(DEV)), 1, hw)
    _, fused, p = _decoder("fused")
    got = _run(fused, p, x, 1, hw)
    assert torch.isfinite(got).all()
    rows = sorted({0, hw - 1} | set(range(7, hw, 32)[:510]))
    assert len(rows) == 512
    err = rel_l2(got[rows], _block_ref(cfg, p, x, 1, hw, rows=torch.tensor(rows)))
    print(f"fused mid-block attention hw={hw}: {err:.2e} vs fp64 on {len(rows)} rows")
    assert err <= 2e-2


# ------------------------------------------------------------------------------------------------ refusals and routing
def test_refusals_launch_nothing():
    from vdpp_amd import hip
    from vdpp_amd.models.vae_hip import TemporalDecoderHIP, VAEDecoderConfig, random_state_dict
    lib = hip.load()
    t = torch.zeros(64, 512, dtype=torch.float16, device=DEV)
    o = torch.full((64, 512), 7.0, dtype=torch.float16, device=DEV)
    a = (t.data_ptr(), t.data_ptr(), t.data_ptr(), o.data_ptr())
    for args, msg in (((*a, 512, 512, 512, 512, None, 1, 64, 64, 0.1, None), b"head_dim 64"),
                      ((*a, 512, 512, 512, 512, None, 1, 64, 192, 0.1, None), b"head_dim 192"),
                      ((*a, 512, 512, 512, 512, None, 1, 0, 512, 0.1, None), b"must be positive"),
                      ((*a, 512, 504, 512, 512, None, 1, 64, 512, 0.1, None), b"at least head_dim"),
                      ((None, *a[1:], 512, 512, 512, 512, None, 1, 64, 512, 0.1, None), b"null pointer")):
        assert lib.sp_attn_wide_f16(*args) < 0 and msg in lib.sp_last_error(), msg
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    cfg = VAEDecoderConfig(block_out_channels=(64, 64, 64, 64))
    with pytest.raises(ValueError, match='attention="composed"'):
        TemporalDecoderHIP(cfg, random_state_dict(cfg, seed=1), DEV, attention="fused")._check_tokens(256)
    with pytest.raises(ValueError, match="'composed' or 'fused'"):
        TemporalDecoderHIP(VAEDecoderConfig.tiny(64), random_state_dict(VAEDecoderConfig.tiny(64), seed=1), DEV, attention="flash")


def test_generate_with_fused_vae_attention(monkeypatch, tmp_path):
    """``--vae-attention fused`` reaches the encoder and the decoder (both call ``ops.attn_wide``), and the file is written."""
    Image = pytest.importorskip("PIL.Image")
    from vdpp_amd.hip import ops
    from vdpp_amd.modes import generate
    calls, real = [], ops.attn_wide
    monkeypatch.setattr(ops, "attn_wide", lambda *a, **kw: (calls.append(kw["seq"]), real(*a, **kw))[1])
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    src = tmp_path / "in.png"
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (64, 128, 3), dtype=np.uint8)).save(src)
    out = tmp_path / "out.npy"
    generate.main(["--backend", "gloo", "--init-method", f"file://{tmp_path}/rendezvous_wide", "--log-level", "WARNING",
                   "--random-init", "--tiny", "--input-image", str(src), "--height", "64", "--width", "128", "--num-frames", "2",
                   "--total-steps", "2", "--vae-attention", "fused", "--output", str(out)])
    assert not torch.distributed.is_initialized()
    assert len(calls) >= 2 and set(calls) == {128}, calls
    frames = np.load(out)
    assert frames.shape[-4:] == (2, 64, 128, 3) and frames.dtype == np.uint8 and int(frames.max()) > int(frames.min())
