"""Whole-model parity of the three edge engines that can see their attention: ``TemporalDecoderHIP``, ``ImageEncoderHIP``
and ``CLIPVisionHIP`` against their fp32 oracles under the peaked state dicts of tests/edge_mutants.py (softmax rows with
a dominant key, AlphaBlender weights 0.12 ... 0.88 with mixed signs), judged at the final output, at every captured
block's output and at every block's branch (output - input).

Bounds: ``T = 3 x`` the error of the oracle's fp16-storage emulation (the output of every Linear / Conv / GroupNorm /
LayerNorm rounded to fp16) for the same quantity on the same inputs -- computed here from the oracle alone, never from
the engine; FACTOR = 3 is the project's own (tests/unet_mutants.py).  Measured on one MI355X the engines stand at 0.34 to
0.71 T over all 257 quantities compared (1.0 to 2.1 x the emulation; the closest is one image of the small CLIP), so the
emulation needed none of the engines' further roundings (fp16 logits on the fp16-score route, P and V^T in fp16, the
folded LayerNorm) and FACTOR stays as it is.  tests/test_edge_sensitivity_cpu.py shows on the CPU
that every mutant of tests/edge_mutants.py moves the quantity compared here by at least 2 T at exactly these shapes
(table: profiles/edge_sensitivity.txt).  Every test prints the measured error beside its bound, per block (pytest -s;
recorded in profiles/edge_parity.txt)."""
import pytest
import torch

from tests import edge_mutants as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def engines():
    built = {}

    def get(case):
        key = case.oracle_key
        if key not in built:
            from vdpp_amd.models.clip_hip import CLIPVisionHIP, CLIPVisionSpec
            from vdpp_amd.models.vae_hip import ImageEncoderHIP, TemporalDecoderHIP
            sd = M.peaked_state_dict(case)
            if case.model == "clip":
                hip = CLIPVisionHIP(CLIPVisionSpec.from_config(M.clip_config(case.kind)), sd, DEV)
            else:
                hip = (TemporalDecoderHIP if case.model == "decoder" else ImageEncoderHIP)(M.vae_configs()[0], sd, DEV)
            built[key] = (M.peaked_oracle(key), hip)
        return built[key]
    return get


def _compare(ref, hip, case):
    x = M.case_inputs(case)
    want, blocks, noise = M.noise_and_bounds(ref, case, x)
    with M.capture_engine(hip) as seen:
        got = M.run_engine(hip, case, x.to(DEV))
    torch.cuda.synchronize()
    got = got.float().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    M.assert_same_blocks(seen, blocks)

    err, t = M.rel_l2(got, want), M.FACTOR * noise["final"]
    print(f"\n{case.name}: final output rel-L2 {err:.2e}  (T = {t:.2e})")
    print(f"  {'block':<36s} {'output':>9s} {'T':>9s}   {'branch':>9s} {'T':>9s}")
    late_out, late_branch = {}, {}
    for i, (e, o) in enumerate(zip(seen, blocks)):
        e_out, t_out = M.rel_l2(e.y, o.y), M.FACTOR * noise["out"][i]
        e_br, t_br = M.rel_l2(e.branch.cpu(), o.branch), M.FACTOR * noise["branch"][i]
        print(f"  {i:2d} {o.name:<33s} {e_out:9.2e} {t_out:9.2e}   {e_br:9.2e} {t_br:9.2e}")
        if e_out > t_out:
            late_out[f"{i} {o.name}"] = f"{e_out:.2e} > {t_out:.2e}"
        if e_br > t_br:
            late_branch[f"{i} {o.name}"] = f"{e_br:.2e} > {t_br:.2e}"
    assert err <= t, f"final output rel_l2={err:.3e}, T={t:.3e}"
    for v in range(case.b) if case.b > 1 else ():       # each item / video / image within its own T
        rows = want.shape[0] // case.b
        sel = slice(v * rows, (v + 1) * rows)
        e_v, t_v = M.rel_l2(got[sel], want[sel]), M.FACTOR * M.rel_l2(noise["emu"][sel], want[sel])
        print(f"  item {v}: {e_v:.2e}  (T = {t_v:.2e})")
        assert e_v <= t_v, f"item {v}: rel_l2={e_v:.3e}, T={t_v:.3e}"
    assert not late_out, f"block outputs beyond their bound: {late_out}"
    assert not late_branch, f"block branches beyond their bound: {late_branch}"


@pytest.mark.parametrize("name", [n for n, c in M.CASES.items() if c.model == "decoder"])
def test_decoder_peaked_weights_match_oracle_at_every_block(engines, name):
    """``decode`` on the fp16-score route (128 tokens a frame), on the fp32-score route (256) and with two items in one
    call; ``decode_latents`` with chunks that straddle the two videos (4) and with one chunk (14)."""
    _compare(*engines(M.CASES[name]), M.CASES[name])


@pytest.mark.parametrize("chunk", [4, 14])
def test_decoder_uint8_frames_equal_the_converted_fp32_frames(engines, chunk):
    """``decode_latents_uint8`` byte for byte ``frames_to_uint8(decode_latents(...))`` under the peaked weights."""
    from vdpp_amd.models.image_io import frames_to_uint8
    case = M.CASES[f"latents 2x3x8x8 chunk {chunk}"]
    _, hip = engines(case)
    lat = M.case_inputs(case).to(DEV)
    want = frames_to_uint8(hip.decode_latents(lat, case.f, decode_chunk_size=chunk))
    got = hip.decode_latents_uint8(lat, case.f, decode_chunk_size=chunk)
    torch.cuda.synchronize()
    assert got.shape == (case.b, case.f, 8 * case.h, 8 * case.w, 3) and got.dtype == torch.uint8
    assert int(got.max()) > int(got.min())
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", [n for n, c in M.CASES.items() if c.model == "encoder"])
def test_encoder_peaked_weights_match_oracle_at_every_block(engines, name):
    """Two images of 128 (fp16 scores) and of 256 (fp32 scores) mid-block tokens."""
    _compare(*engines(M.CASES[name]), M.CASES[name])


@pytest.mark.parametrize("name", [n for n, c in M.CASES.items() if c.model == "clip"])
def test_clip_peaked_weights_match_transformers_at_every_layer(engines, name):
    """The small configuration and a shallow ViT-H/14 (head width 80, 257 keys): the hidden state of all tokens behind
    every layer, every layer's branch, and ``image_embeds``."""
    _compare(*engines(M.CASES[name]), M.CASES[name])
