"""The draw generators of tools/fuzz_misc.py for the newer kernels (``draw_new``), run on the CPU with no kernel: the very
series tests/test_fuzz_gpu.py::test_new_kernel_fuzz runs.  Every reference is finite, every integer-operand reference of
sp_gemm_f8 and every cell mean of sp_kv_pool_f16 is exactly representable in fp16 (so "equal" is a fair demand), every
pitch rule of the entry points is met, and the series has the coverage the GPU test asserts."""
import collections
import os
import random
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_new_kernel_draws_are_finite_exact_and_cover_the_grid():
    import fuzz_misc as Z
    rng, g = random.Random(Z.NEW_SEED), torch.Generator().manual_seed(Z.NEW_SEED)
    cases = [Z.draw_new(rng, g, i) for i in range(Z.NEW_DRAWS)]
    kinds = collections.Counter(c["kind"] for c in cases)
    assert set(kinds) == set(Z.NEW_KINDS) and min(kinds.values()) >= 5, kinds
    for c in cases:
        refs = [c["y"], c["st"]] if c["kind"] == "ln_quant_f8" else c["ref"] if isinstance(c["ref"], list) else [c["ref"]]
        assert all(bool(torch.isfinite(r.double()).all()) for r in refs), c["what"]
        if c["kind"] == "gemm_f8" and c["mode"] != "geglu":
            assert torch.equal(c["ref"].half().double(), c["ref"]), "not representable in fp16: " + c["what"]
        if c["kind"] == "kv_pool":
            for src, ref in zip((c["k"], c["v"]), c["ref"]):
                f = c["factor"]
                exact = src.double().view(c["n_img"], c["h"] // f, f, c["w"] // f, f, c["c"]).mean((2, 4)).reshape(-1, c["c"])
                assert torch.equal(ref.double(), exact.half().double()) and c["h"] != c["w"], c["what"]
    gemms = [c for c in cases if c["kind"] == "gemm_f8"]
    assert sum(min(Z.gemm_f8_tiles(c)) >= 3 for c in gemms) >= 5 and sum(c["k"] == 640 for c in gemms) >= 3
    assert {c["mode"] for c in gemms} == {"plain", "res", "geglu"}
    assert max(tm * tn for tm, tn in map(Z.gemm_f8_tiles, gemms)) <= 25 and any(tm * tn % 2 for tm, tn in map(Z.gemm_f8_tiles, gemms))
    assert {c["factor"] for c in cases if c["kind"] == "kv_pool"} == {2, 4}
    assert {c["d"] for c in cases if c["kind"] == "attn_wide"} == {128, 256, 512}
    assert {c["bias"] is None for c in cases if c["kind"] == "attn_wide"} == {False, True}
    print({k: [c["what"] for c in cases if c["kind"] == k] for k in Z.NEW_KINDS})
