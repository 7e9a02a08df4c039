"""What the peaked-weights parity tests of the edge engines (tests/test_edge_peaked_gpu.py) can see, checked on the CPU with
the fp32 oracles alone: under the peaked state dicts every mutant of tests/edge_mutants.py -- a plausible bug of
``TemporalDecoderHIP`` / ``ImageEncoderHIP`` / ``CLIPVisionHIP``, planted in the oracle -- moves the compared quantity by at
least twice the bound the GPU test allows the engine, at exactly the shapes the GPU test runs.  The bound is ``T = 3 x``
the error of the oracle's fp16-storage emulation for the same quantity.

Conditions (tests/unet_mutants.py: FACTOR = 3, MARGIN = 2):
* outputs finite, noise <= 1e-2 for the final output, every block's output and every block's branch;
* every self-attention has logits of standard deviation >= 2 and a largest probability >= 2 x a flat row's;
* every mutant applied EVERYWHERE moves the final output by >= 2 T;
* every mutant that acts inside a block, applied to ONE block, moves that block's branch (output - input; the output of a
  resnet that changes the width) by >= 2 T of that block;
* the exceptions are exactly the documented ones: a dropped key among 128 or 256 (0.4 to 0.8 % of a row's mass on
  average: key counts are held at kernel level, ``test_attention_small`` / ``test_softmax_rows*``; at 64 keys and in CLIP
  it must show); "across items" where a call has one item; "chunks cut per video" outside ``decode_latents``;
* ``mutate`` and ``fp16_storage`` leave the oracle bit-identical;
* as a record of the state before: with plain random weights at the real widths the attention may be replaced by a mean
  of V, or run with a doubled scale, and the compared output moves by less than the 2e-2 / 1e-2 that
  tests/test_vae_gpu.py / tests/test_clip_gpu.py allow.

``python -m tests.edge_mutants`` prints the whole table (profiles/edge_sensitivity.txt)."""
import pytest
import torch

from tests import edge_mutants as M


@pytest.fixture(scope="module", params=list(M.CASES))
def table(request):
    return M.sensitivity(request.param)


def _drop_key_is_invisible(case):
    """A VAE frame of 128 or 256 tokens: one key carries 1/128 of a flat row and less of a peaked one."""
    tokens = case.h * case.w if case.model == "decoder" else (case.h // 8) * (case.w // 8)
    return case.model != "clip" and tokens >= 128


def test_blocks_are_captured_in_call_order(table):
    case = M.CASES[table["case"]]
    names, kinds = [n for n, _ in table["blocks"]], [k for _, k in table["blocks"]]
    if case.model == "decoder":
        calls = 2 if case.chunk == 4 else 1                                  # chunks of 4 and 2 frames
        one = ["mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"] + \
              [f"up_blocks.{i}.resnets.{j}" for i in range(4) for j in range(3)]
        assert names == one * calls and kinds.count("attn") == calls and kinds.count("res") == 14 * calls
    elif case.model == "encoder":
        assert names == [f"encoder.down_blocks.{i}.resnets.{j}" for i in range(4) for j in range(2)] + \
            ["encoder.mid_block.resnets.0", "encoder.mid_block.attentions.0", "encoder.mid_block.resnets.1"]
        assert kinds == ["res2d"] * 9 + ["attn", "res2d"]
    else:
        layers = M.clip_config(case.kind).num_hidden_layers
        assert names == [f"vision_model.encoder.layers.{i}" for i in range(layers)] and kinds == ["layer"] * layers


def test_outputs_finite_and_fp16_noise_small(table):
    n = table["noise"]
    assert table["finite"]
    worst = max([n["final"]] + n["out"] + n["branch"])
    print(f"{table['case']}: fp16-storage noise final {n['final']:.2e}, worst block quantity {worst:.2e}")
    assert 0 < n["final"] and min(n["out"] + n["branch"]) > 0
    assert worst <= 1e-2, f"fp16 storage alone moves a compared quantity by {worst:.2e}: T means little"


def test_rows_are_peaked(table):
    """The point of the recipe: a self-attention row has a dominant key.  Logits of standard deviation 2 put a factor e^2
    between a typical key and one a standard deviation above it."""
    assert table["peaks"]
    for name, std, pmax, flat in table["peaks"]:
        assert std >= 2.0 and pmax >= 2 * flat, f"{name}: logit std {std:.2f}, largest probability {pmax:.3f} against {flat:.4f}"


def test_every_mutant_applied_everywhere_moves_the_final_output(table):
    case = M.CASES[table["case"]]
    t = M.FACTOR * table["noise"]["final"]
    assert set(table["all"]) == {m.name for m in M.MUTANTS if M.applies(m, case)}
    weak = {name: f"{d / t:.1f} x T" for name, d in table["all"].items() if d < M.MARGIN * t}
    want = {"vae attention: last key dropped"} if _drop_key_is_invisible(case) else set()
    assert set(weak) == want, f"{case.name}: invisible to a final-output bound of {t:.2e}: {weak}; documented: {want}"


def test_every_mutant_in_one_block_moves_that_blocks_branch(table):
    case = M.CASES[table["case"]]
    n, weak, seen = table["noise"], {}, 0
    for mut in M.MUTANTS:
        if mut.drop_key and _drop_key_is_invisible(case):
            continue
        for i, d in table["one"].get(mut.name, {}).items():
            t = M.FACTOR * n["branch"][i]
            seen += 1
            if d < M.MARGIN * t:
                weak[f"{mut.name} in {i} {table['blocks'][i][0]}"] = f"{d / t:.1f} x T"
    blocks = len(table["blocks"])
    assert seen >= {"decoder": 4 * blocks, "encoder": 7, "clip": 6 * blocks}[case.model]
    assert not weak, f"{case.name}: invisible to the block's own bound: {weak}"


def test_mutants_that_cannot_show_are_the_documented_ones(table):
    """Cases a mutant is not asked for: one item per call has nothing to run across, only ``decode_latents`` cuts chunks;
    and inside the blocks, ``conv_shortcut`` exists only where the width changes (up_blocks.2 / .3, first resnet)."""
    case = M.CASES[table["case"]]
    want = []
    if case.model == "decoder":
        if not (case.kind == "decode" and case.b == 2):
            want += ["resblock: temporal half across items", "decoder: time_conv_out across items"]
        if case.kind != "latents":
            want += ["decoder: chunks cut per video"]
    assert sorted(table["skipped"]) == sorted(want)
    for mut in M.MUTANTS:
        if not mut.in_block or mut.name not in table["one"]:
            continue
        kinds = {"vae_attn": ("attn",), "dec_res": ("res",), "clip_attn": ("layer",), "clip_end": ("layer",)}[mut.family]
        hit = [table["blocks"][i][0] for i in table["one"][mut.name]]
        expect = [nm for nm, k in table["blocks"] if k in kinds]
        if mut.what == "noshortcut":
            expect = [nm for nm in expect if nm in ("up_blocks.2.resnets.0", "up_blocks.3.resnets.0")]
        assert hit == expect, mut.name


@pytest.mark.parametrize("name", ["decode 2x3x8x8", "latents 2x3x8x8 chunk 4", "encode 2x64x128", "clip small 2x56"])
def test_mutate_and_fp16_storage_leave_the_oracle_as_it_was(name):
    case = M.CASES[name]
    ref = M.build_oracle(case, M.peaked_state_dict(case))
    x = M.case_inputs(case)
    with M.capture_oracle(ref):               # (transformers hangs its own output-recording hooks on first use: they stay)
        want = M.run_oracle(ref, case, x)

    def patches():
        return [(len(m._forward_hooks), len(m._forward_pre_hooks), "forward" in m.__dict__) for m in ref.modules()]
    before, hooks = {k: v.clone() for k, v in ref.state_dict().items()}, patches()
    assert case.model == "clip" or not any(any(p) for p in hooks)
    for mut in M.MUTANTS:
        if M.applies(mut, case):
            with M.mutate(ref, mut) as hit:
                assert hit
                assert not torch.equal(M.run_oracle(ref, case, x), want), mut.name
    with M.fp16_storage(ref), M.capture_oracle(ref) as rec:
        assert not torch.equal(M.run_oracle(ref, case, x), want) and rec
    assert torch.equal(M.run_oracle(ref, case, x), want)
    assert all(torch.equal(v, before[k]) for k, v in ref.state_dict().items())
    assert patches() == hooks
    assert "_chunks_per_video" not in ref.__dict__


def test_plain_random_weights_hide_the_attention_at_the_real_widths():
    """The state before: the two real-width rows of the issue's table stay under the bounds of the existing tests."""
    rec = M.plain_weights_record()
    dec, clip = rec["decoder, SVD widths, 2 x 24 x 32 latent"], rec["clip, ViT-H/14 widths, 257 tokens, 4 layers"]
    for r in (dec, clip):
        print({k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in r.items()})
        assert all(std < 0.5 and pmax < 5 * flat for _, std, pmax, flat in r["peaks"])
    assert dec["fp16-storage noise"] < dec["vae attention: softmax -> mean of V"] < 2e-2
    assert dec["fp16-storage noise"] < dec["vae attention: logits x2"] < 2e-2
    assert clip["fp16-storage noise"] < clip["clip: softmax -> mean of V"] < 1e-2
    assert clip["fp16-storage noise"] < clip["clip: scale x2"] < 1e-2
