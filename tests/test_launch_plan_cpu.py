"""Which norm sites take which path, pinned without a GPU.

The engines never compute with torch: they allocate and call ``hip.ops`` wrappers.  With every wrapper replaced by a
recorder, the stream queries stubbed and the device check (``models.common.hip_device``) replaced, a whole forward runs
on CPU tensors and yields its list of launches.  Per configuration the tests assert

* how many launches of each kind a forward makes (recorded before the statistics hand-off became explicit data flow;
  a fusion that silently falls back to a statistics pass passes every parity test and only gets slower -- here it fails),
* that a norm which skips its statistics pass reads the statistics of the contraction that wrote its input: the very
  ``gn_part`` tensor of that contraction (for a concatenation buffer: of both), and row by row the ``ln_out`` rows that
  belong to the rows of its operand, computed for the same eps -- also where a feed-forward pair ran in row chunks.

Nothing is launched and nothing is computed; every tensor of a forward is kept alive in the log, so addresses identify
buffers."""
import collections

import pytest
import torch

from tests import launch_recorder
from vdpp_amd.models import common, unet_hip, vae_hip
from vdpp_amd.models.unet_spec import UNetConfig, random_state_dict


@pytest.fixture
def log(monkeypatch):
    """The list of launches; the engines build and run on the CPU while it is active."""
    return launch_recorder.install(monkeypatch.setattr)


def counts(log):
    """(gemm, groupnorm, groupnorm_tile_sums, ... with part_b, groupnorm_fold_linear_tile_sums, ln_stats, gemm_f32out,
    gemm with gn_part, ... with ln_out, ... with w_group_rows)"""
    n = collections.Counter(l.name for l in log)
    gemms = [l for l in log if l.name == "gemm"]
    return (n["gemm"], n["groupnorm"], n["groupnorm_tile_sums"],
            sum(l.name == "groupnorm_tile_sums" and l.kw.get("part_b") is not None for l in log),
            n["groupnorm_fold_linear_tile_sums"], n["ln_stats"], n["gemm_f32out"],
            sum(l.kw.get("gn_part") is not None for l in gemms), sum(l.kw.get("ln_out") is not None for l in gemms),
            sum(bool(l.kw.get("w_group_rows")) for l in gemms))


def same_memory(t, ptr, shape):
    return t.data_ptr() == ptr and tuple(t.shape) == tuple(shape)


def writer(log, before, ptr, shape):
    """The last contraction in front of launch ``before`` whose destination is exactly that memory."""
    for l in reversed(log[:before]):
        if l.name == "gemm" and same_memory(l.args[2], ptr, shape):
            return l
    raise AssertionError(f"no contraction wrote the {tuple(shape)} operand of launch {before} ({log[before].name})")


def check_tile_sums_come_from_the_producer(log):
    """Returns how many consumers were checked."""
    checked = 0
    for i, l in enumerate(log):
        if l.name == "groupnorm_tile_sums":
            x, part = l.args[0], l.args[1]
            if l.kw.get("part_b") is not None:      # a concatenation buffer: left and right halves, one producer each
                c_a = l.kw["c_a"]
                assert x.stride(0) == x.shape[1] and l.kw["ldx"] == x.shape[1]
                assert writer(log, i, x.data_ptr(), (x.shape[0], c_a)).kw.get("gn_part") is part
                assert writer(log, i, x.data_ptr() + 2 * c_a, (x.shape[0], x.shape[1] - c_a)).kw.get("gn_part") is l.kw["part_b"]
            else:
                assert writer(log, i, x.data_ptr(), x.shape).kw.get("gn_part") is part
            assert l.kw["rows"] % 256 == 0
            checked += 1
        elif l.name == "groupnorm_fold_linear_tile_sums":   # the folded weights go to the next launch, a contraction on x
            user = log[i + 1]
            assert user.name == "gemm" and user.args[1] is l.args[5] and user.kw["w_group_rows"] == l.kw["rows"]
            x = user.args[0]
            assert writer(log, i, x.data_ptr(), x.shape).kw.get("gn_part") is l.args[0]
            assert l.kw["rows"] % 256 == 0
            checked += 1
    return checked


def check_row_statistics_belong_to_the_operand(log):
    """Every contraction with a folded LayerNorm: row i of its ``ln_stats`` was written -- by a statistics pass or by a
    contraction's ``ln_out`` -- for the very memory of row i of its operand, with the folded LayerNorm's eps.  Returns how
    many consumers read epilogue statistics."""
    wrote = {}                                      # address of a statistics row -> (address of its activation row, eps, by)
    from_epilogue = 0

    def note(stats, act, eps, by):
        assert stats.dtype == torch.float32 and stats.stride() == (2, 1) and stats.shape[0] == act.shape[0]
        for i in range(stats.shape[0]):
            wrote[stats.data_ptr() + 8 * i] = (act.data_ptr() + 2 * act.stride(0) * i, eps, by)

    for l in log:
        if l.name == "ln_stats":
            note(l.args[1], l.kw.get("sum_out") if l.kw.get("sum_out") is not None else l.args[0], l.kw["eps"], "pass")
        if l.name != "gemm":
            continue
        st = l.kw.get("ln_stats")
        if st is not None:
            a, m = l.args[0], l.kw["m"]
            assert l.kw["ln_colsum"] is not None and st.shape == (m, 2) and a.shape[0] == m
            rows = [wrote.get(st.data_ptr() + 8 * i) for i in range(m)]
            assert None not in rows, f"{rows.count(None)} of {m} statistics rows were never written"
            assert all(r[0] == a.data_ptr() + 2 * a.stride(0) * i for i, r in enumerate(rows))
            assert {r[1] for r in rows} == {1e-5}
            from_epilogue += rows[0][2] == "epilogue"
        if l.kw.get("ln_out") is not None:
            note(l.kw["ln_out"], l.args[2], l.kw["ln_out_eps"], "epilogue")
    return from_epilogue


def run_unet(log, c, shape, *, chunks=None, euler=False):
    cfg = UNetConfig.tiny(c)
    hip = unet_hip.SVDUNetHIP(cfg, random_state_dict(cfg, seed=47, dtype=torch.float16), "cpu")
    if chunks:
        hip.FF_CHUNK_BYTES, hip.FF_CHUNK_ROUND = chunks
    log.clear()
    b, f, _, h, w = shape
    ctx = torch.zeros(b, 1, cfg.cross_attention_dim).half()
    ids = torch.tensor([[5.0, 127.0, 0.02]] * b)
    if euler:
        e = dict(latent=torch.zeros(b, 4, f, h, w).half(), out=torch.zeros(b, 4, f, h, w).half(), sigma=torch.zeros(1),
                 sigma_next=torch.zeros(1))
        got = hip.forward_rows(torch.zeros((b * f * h * w, hip.cin_pad), dtype=torch.float16), b=b, frames=f, h=h, w=w,
                               t_value=torch.zeros(1), ctx16=ctx.reshape(b, -1), added_ids32=ids[0], euler=e)
        assert got is None and "euler" in log[-1].kw
    else:
        out = hip(torch.zeros(shape).half(), 0.6, ctx, ids)[0]
        assert type(out) is torch.Tensor and out.shape == (b, f, 4, h, w)
    return hip


#                                   gemm  gn  tile_sums (part_b)  fold  ln_stats  f32out  gemm with gn_part / ln_out / w_groups
UNET_PLANS = [
    (256, (2, 3, 8, 16, 16), None, (302, 79, 21, 3, 5, 40, 0, 27, 40, 5)),
    (64, (1, 3, 8, 16, 24), None, (302, 105, 0, 0, 0, 56, 0, 0, 24, 0)),                  # no tile fits: every norm runs its pass
    (256, (1, 2, 8, 32, 32), None, (302, 54, 41, 6, 10, 40, 0, 53, 40, 10)),              # two levels of whole tiles
    (256, (2, 3, 8, 16, 16), (1 << 18, 256), (482, 79, 21, 3, 5, 40, 0, 27, 70, 5)),      # feed-forward pairs in row chunks
]


@pytest.mark.parametrize("c,shape,chunks,want", UNET_PLANS)
def test_unet_launch_plan(log, c, shape, chunks, want):
    run_unet(log, c, shape, chunks=chunks)
    assert counts(log) == want
    # (a few contractions are asked for column sums that no norm folds, e.g. 27 written and 26 read in the first plan)
    assert check_tile_sums_come_from_the_producer(log) == want[2] + want[4]
    # 80 folded LayerNorms per forward (16 transformers x 5); those without a statistics pass read an epilogue's rows
    folded = [(i, l) for i, l in enumerate(log) if l.name == "gemm" and l.kw.get("ln_stats") is not None]
    from_epilogue = check_row_statistics_belong_to_the_operand(log)
    if chunks is None:
        assert len(folded) == 80 and from_epilogue == 80 - want[5]
        # unchunked, the hand-off is one object: ln_stats of the consumer IS ln_out of the contraction that wrote its operand
        passes = {id(l.args[1]) for l in log if l.name == "ln_stats"}
        handed = [(i, l) for i, l in folded if id(l.kw["ln_stats"]) not in passes]
        assert len(handed) == 80 - want[5]
        for i, l in handed:
            assert writer(log, i, l.args[0].data_ptr(), l.args[0].shape).kw.get("ln_out") is l.kw["ln_stats"]
    else:
        rows = shape[0] * shape[1] * shape[3] * shape[4]
        assert any(l.kw["geglu"] and l.kw["m"] < rows for _, l in folded), "no feed-forward was chunked"
        assert any(l.kw.get("ln_out") is not None and l.kw["m"] < rows for l in log if l.name == "gemm")
        assert from_epilogue >= 80 - want[5]


def test_unet_launch_plan_with_euler_epilogue(log):
    """The fused Euler update changes the last contraction only."""
    run_unet(log, 256, (2, 3, 8, 16, 16), euler=True)
    assert counts(log) == UNET_PLANS[0][3]
    assert check_tile_sums_come_from_the_producer(log) == 26


@pytest.mark.parametrize("switch,want", [
    ("VDPP_GN_EPILOGUE", (302, 100, 0, 0, 0, 40, 0, 0, 40, 5)),
    ("VDPP_GN_EPILOGUE_RES", (302, 89, 11, 0, 0, 40, 0, 12, 40, 5)),
    ("VDPP_FOLD_GN", (302, 79, 26, 3, 0, 40, 0, 27, 40, 0)),
    ("VDPP_FOLD_SHORTCUT", (302, 79, 21, 3, 5, 40, 0, 27, 40, 5)),
    ("VDPP_LN_OUT_WIDE", (302, 79, 21, 3, 5, 40, 0, 27, 40, 5)),
])
def test_unet_launch_plan_with_a_switch_off(log, monkeypatch, switch, want):
    monkeypatch.setenv(switch, "0")
    run_unet(log, 256, (2, 3, 8, 16, 16))
    assert counts(log) == want
    assert check_tile_sums_come_from_the_producer(log) == want[2] + want[4]
    assert check_row_statistics_belong_to_the_operand(log) == 40


def test_chunked_feed_forward_leaves_row_statistics_for_all_rows_or_none(log):
    """A feed-forward pair in row chunks whose second contraction has three or four column tiles per row (768 ... 1,280
    channels) leaves the next LayerNorm's statistics only from more than SPLITK_MAX_ROWS rows: with a short last chunk
    no chunk writes any, the output carries none and its consumer runs the statistics pass."""
    cfg = UNetConfig.tiny(64)
    hip = unet_hip.SVDUNetHIP(cfg, random_state_dict(cfg, seed=0, dtype=torch.float16), "cpu")
    c, m = 768, 16384
    ff1 = common._Dense.fold_layernorm(torch.zeros(8 * c, c), torch.zeros(8 * c), torch.ones(c), torch.zeros(c), "cpu",
                                       eps=1e-5, geglu=True)
    ff2 = common._Dense(torch.zeros(c, 4 * c, dtype=torch.float16), torch.zeros(c), cin=4 * c)
    nxt = common._Dense.fold_layernorm(torch.zeros(c, c), None, torch.ones(c), torch.zeros(c), "cpu", eps=1e-5)
    run = unet_hip._Run(b=1, f=1, h=128, w=128, temb=None, ctx16=None, gn_ws=None, sk_ws=None, frame_ids=None)
    x = torch.empty(m, c, dtype=torch.float16)
    assert hip.SPLITK_MAX_ROWS == 6144
    for rows, hands_over in ((8192, True), (6400, False), (4096, False)):      # chunks of 8192+8192, 6400+6400+3584, 4 x 4096
        hip.FF_CHUNK_BYTES, hip.FF_CHUNK_ROUND = rows * 4 * c * 2, 256
        log.clear()
        st = hip._ln_pass(ff1, x)
        out = hip._ff_pair(run, ff1, ff2, x, st, ln_next=nxt, res1=x, r1scale=1.0)
        second = [l for l in log if l.name == "gemm" and not l.kw["geglu"]]
        assert [l.kw["m"] for l in second] == [min(rows, m - r0) for r0 in range(0, m, rows)]
        assert [l.kw.get("ln_out") is not None for l in second] == [hands_over] * len(second)
        assert (out.ln_stats is not None) == hands_over
        qkv = hip._gemm(run, nxt, out.t, ln_stats=hip._ln_stats(nxt, out))
        assert qkv.t.shape == (m, c) and [l.name for l in log[-2:]] == (["gemm", "gemm"] if hands_over else ["ln_stats", "gemm"])
        assert check_row_statistics_belong_to_the_operand(log) == int(hands_over)


VAE_PLANS = [
    ((2, 4, 8, 8), (72, 45, 13, 0, 0, 0, 0, 13, 0, 0)),
    ((4, 4, 16, 16), (74, 24, 34, 0, 0, 0, 4, 34, 0, 0)),
]


@pytest.mark.parametrize("zshape,want", VAE_PLANS)
def test_vae_decoder_launch_plan(log, zshape, want):
    cfg = vae_hip.VAEDecoderConfig.tiny(64)
    dec = vae_hip.TemporalDecoderHIP(cfg, vae_hip.random_state_dict(cfg, seed=1), "cpu")
    log.clear()
    out = dec.decode(torch.zeros(zshape).half(), 2)
    assert type(out) is torch.Tensor and out.shape == (zshape[0], 3, 8 * zshape[2], 8 * zshape[3])
    assert counts(log) == want
    assert check_tile_sums_come_from_the_producer(log) == want[2] == want[7]


def test_vae_image_encoder_launch_plan(log):
    cfg = vae_hip.VAEDecoderConfig.tiny(64)
    enc = vae_hip.ImageEncoderHIP(cfg, vae_hip.random_encoder_state_dict(cfg, seed=2), "cpu")
    log.clear()
    out = enc.encode_image_latents(torch.zeros(2, 3, 128, 128).half(), 3)
    assert type(out) is torch.Tensor and out.shape == (2, 4, 3, 16, 16)
    # only the attention's output projection is asked for column sums (the encoder's resnets are not)
    assert counts(log) == (34, 21, 1, 0, 0, 0, 2, 1, 0, 0)
    assert check_tile_sums_come_from_the_producer(log) == 1


def test_no_engine_builds_without_a_hip_device():
    """The shared device check: same exception for the three engines, before anything is loaded."""
    from vdpp_amd.models import clip_hip
    for build, name in ((lambda: unet_hip.SVDUNetHIP(UNetConfig.tiny(64), {}, "cpu"), "SVDUNetHIP"),
                        (lambda: vae_hip.TemporalDecoderHIP(vae_hip.VAEDecoderConfig.tiny(64), {}, "cpu"), "TemporalDecoderHIP"),
                        (lambda: vae_hip.ImageEncoderHIP(vae_hip.VAEDecoderConfig.tiny(64), {}, "cpu"), "ImageEncoderHIP"),
                        (lambda: clip_hip.CLIPVisionHIP(clip_hip.CLIPVisionSpec.svd(), {}, "cpu"), "CLIPVisionHIP")):
        with pytest.raises(RuntimeError, match=f"{name} runs on an MI355X HIP device only"):
            build()
