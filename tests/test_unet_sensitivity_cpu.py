"""What the peaked-weights UNet parity tests (tests/test_unet_peaked_gpu.py) can see, checked on the CPU with the fp32
oracle alone: under ``peaked_state_dict`` every mutant of tests/unet_mutants.py -- a plausible engine bug, planted in the
oracle -- moves the compared quantity by at least twice the bound the GPU test allows the engine, at exactly the shapes the
GPU test runs.  The bound is ``T = 3 x`` the error of the oracle's fp16-storage emulation for the same quantity.

Conditions (tests/unet_mutants.py: FACTOR = 3, MARGIN = 2):
* outputs finite, noise <= 1e-2 for the final output, every block's output and every transformer's branch;
* every mutant applied to ALL blocks moves the final output by >= 2 T;
* every mutant but the dropped keys, applied to ONE transformer, moves that block's branch by >= 2 T of that block
  (a dropped key in one block need not show: key counts are visible at kernel level, where a flat softmax makes one key
  in 1,000 a 3 % error; mutants that change nothing in a block -- head rotation with one head, a spatial softmax over
  one token -- are not asked for there);
* as a record of the state before: with plain ``random_state_dict`` the temporal softmax may be replaced by a mean in all
  16 transformers and the output moves by less than the 2e-2 that tests/test_unet_gpu.py allows.

``python -m tests.unet_mutants`` prints the whole table (profiles/unet_sensitivity.txt)."""
import pytest
import torch

from tests import unet_mutants as M


@pytest.fixture(scope="module", params=list(M.CASES))
def table(request):
    return M.sensitivity(request.param)


def test_blocks_are_captured_in_call_order(table):
    kinds = [k for _, k in table["blocks"]]
    names = [n for n, _ in table["blocks"]]
    assert kinds.count("res") == 22 and kinds.count("xf") == 16
    assert names[:4] == ["down_blocks.0.resnets.0", "down_blocks.0.attentions.0", "down_blocks.0.resnets.1",
                         "down_blocks.0.attentions.1"]
    assert names[12:17] == ["down_blocks.3.resnets.0", "down_blocks.3.resnets.1", "mid_block.resnets.0",
                            "mid_block.attentions.0", "mid_block.resnets.1"]
    assert names[-1] == "up_blocks.3.attentions.2"


def test_outputs_finite_and_fp16_noise_small(table):
    n = table["noise"]
    assert table["finite"]
    worst = max([n["final"]] + n["out"] + [x for x in n["branch"] if x is not None])
    print(f"{table['case']}: fp16-storage noise final {n['final']:.2e}, worst block quantity {worst:.2e}")
    assert 0 < n["final"] and worst <= 1e-2, f"fp16 storage alone moves a compared quantity by {worst:.2e}: T means little"


def test_rows_are_peaked(table):
    """The point of the recipe: a self-attention row has a dominant key.  Logits of standard deviation 2 put a factor
    e^2 between a typical key and one a standard deviation above it; the largest probability of a row is then at least
    twice the 1 / n of a plain average (with 3 frames it cannot be more than three times)."""
    for fam, (std, pmax, flat) in table["peaks"].items():
        assert std >= 2.0 and pmax >= 2 * flat, f"{fam}: logit std {std:.2f}, largest probability {pmax:.3f} against {flat:.3f}"


def test_every_mutant_in_all_blocks_moves_the_final_output(table):
    t = M.FACTOR * table["noise"]["final"]
    videos = M.CASES[table["case"]][0]
    assert set(table["all"]) == {m.name for m in M.MUTANTS if videos == 2 or m.what != "video"}
    weak = {name: f"{d / t:.1f} x T" for name, d in table["all"].items() if d < M.MARGIN * t}
    assert not weak, f"{table['case']}: invisible to a final-output bound of {t:.2e}: {weak}"


def test_every_mutant_in_one_block_moves_that_blocks_branch(table):
    n, weak, seen = table["noise"], {}, 0
    for mut in M.MUTANTS:
        if mut.drop_key or mut.family == "control":
            continue
        for i, d in table["one"].get(mut.name, {}).items():
            t = M.FACTOR * n["branch"][i]
            seen += 1
            if d < M.MARGIN * t:
                weak[f"{mut.name} in {table['blocks'][i][0]}"] = f"{d / t:.1f} x T"
    assert seen >= 16 * 7                  # the seven mutants that apply to every transformer, at the least
    assert not weak, f"{table['case']}: invisible to the block's own bound: {weak}"


def test_mutants_that_cannot_show_are_the_documented_ones(table):
    """'-' cells of the table: head rotation where the level has one head (levels 0: six transformers), and at one token per
    frame (8 x 8 latents: the mid block) the spatial softmax mutants and the neighbouring pixel."""
    xf = [i for i, (_, k) in enumerate(table["blocks"]) if k == "xf"]
    one_token = M.CASES[table["case"]][2:] == (8, 8)
    for mut in M.MUTANTS:
        if mut.family == "control" or (mut.what == "video" and M.CASES[table["case"]][0] != 2):
            continue
        missing = [table["blocks"][i][0] for i in xf if i not in table["one"][mut.name]]
        want = []
        if mut.what == "heads":
            want = [n for n, k in table["blocks"] if k == "xf" and n.startswith(("down_blocks.0.", "up_blocks.3."))]
        elif one_token and M.is_identity(mut, 1):
            want = ["mid_block.attentions.0"]
        assert sorted(missing) == sorted(want), mut.name


def test_mutate_and_fp16_storage_leave_the_oracle_as_it_was():
    cfg, _ = M.configs()
    ref = M.build_oracle(M.peaked_state_dict(cfg, M.SEED))
    sample, ctx, ids = M.case_inputs(cfg, "2x3x16x24")
    want = M.run_oracle(ref, sample, ctx, ids)
    for mut in M.MUTANTS:
        with M.mutate(ref, mut, 2, block=None if mut.family != "pos" else "mid_block.attentions.0") as hit:
            assert hit
    with M.fp16_storage(ref), M.capture_oracle(ref) as rec:
        assert not torch.equal(M.run_oracle(ref, sample, ctx, ids), want) and len(rec) == 38
    assert torch.equal(M.run_oracle(ref, sample, ctx, ids), want)
    assert not any(m._forward_hooks or m._forward_pre_hooks or "forward" in m.__dict__ for m in ref.modules())


def test_plain_random_weights_hide_the_temporal_softmax():
    rec = M.plain_weights_record()
    std, pmax, flat = rec["peaks"]["temporal"]
    print(f"plain random_state_dict: temporal logit std {std:.2f}, largest probability {pmax:.3f} (average: {flat:.3f}); "
          f"all-block mean-of-V mutants move the output by {rec['temporal softmax -> mean of V']:.2e} (temporal), "
          f"{rec['spatial softmax -> mean of V']:.2e} (spatial)")
    assert std < 0.5 and pmax < 2 * flat
    assert rec["temporal softmax -> mean of V"] < 2e-2
