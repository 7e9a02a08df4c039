"""What the bit-exact GPU tests (tests/test_gemm_exact_gpu.py, tests/test_attention_exact_gpu.py) can see, shown on the CPU.

Contractions.  On every draw of the GPU series an emulation of a kernel -- fp16 operands, fp32 accumulation over K in a
shuffled order of 64-wide chunks, split into 1 to 4 partial slabs that are summed at the end -- equals the integer
reference bit for bit: the result does not depend on the order of summation, so the tests never need retuning.  Seven
plausible indexing bugs, planted in the operand matrix, each change at least one stored value on every draw they apply to.
The first two are ALSO run with the fuzz's Gaussian operands at the shapes where they were first measured, and pass the
fuzz's 3e-3 on the global and the worst-block error: the reason for the exact tests.

Attention.  fp32 statements of the three kernels' rounding points pass every pattern at every size of the GPU tests, and
each of eight indexing bugs breaks the criterion in at least one pattern at every size where it applies."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_patterns as P  # noqa: E402
import gemm_model as M  # noqa: E402


# ------------------------------------------------------------------------------------------------ contractions
def emulate(d, views, x, rng):
    """fp32 accumulation of fp16 operands over shuffled 64-wide K chunks in 1 to 4 slabs, the fold and the epilogue."""
    m, kk = x.shape
    x = x.float()
    chunks = list(range(0, kk, 64))
    rng.shuffle(chunks)
    nslab = rng.randint(1, 4)

    def contract(xg, wg):
        slabs = [torch.zeros(xg.shape[0], wg.shape[0]) for _ in range(nslab)]
        for i, c in enumerate(chunks):
            slabs[i % nslab] += xg[:, c:c + 64] @ wg[:, c:c + 64].t()
        acc = slabs[0]
        for s in slabs[1:]:
            acc = acc + s
        return acc
    w = views["w"].float()
    if d["w_group_rows"]:
        r = d["w_group_rows"]
        acc = torch.cat([contract(x[g * r:(g + 1) * r], w[g]) for g in range((m + r - 1) // r)], dim=0)
    else:
        acc = contract(x, w[0])
    if d["ln_stats"]:
        st = views["ln_stats"]
        acc = (acc - st[:m, 0:1] * views["ln_colsum"]) * st[:m, 1:2]
    assert acc.dtype == torch.float32
    return M.epilogue(d, views, acc)["d"]


def stored_weights(d, views, row):
    """The weights row ``row`` meets, stored columns only: [columns][K]."""
    g = row // d["w_group_rows"] if d["w_group_rows"] else 0
    return views["w"][g][:M.stored(d)].float()


def _visible_k(d, views, row, ks):
    """First k of ``ks`` whose weight is non-zero in some stored column."""
    w = stored_weights(d, views, row)
    for k in ks:
        if bool((w[:, k] != 0).any()):
            return k
    raise AssertionError("no stored column has a weight there")


def mutate(name, d, views, x, k=None):
    """The mutant's operand matrix and tensors, or None where it does not apply (``k``: the element of the first two)."""
    m, kk = x.shape
    cin, taps = d["cin"], M.TAPS[d["mode"]]
    row = m // 2
    x = x.clone()
    if name == "one (row, k) element read as zero":
        ks = [k] if k is not None else [k for k in range(kk // 3, kk) if x[row, k] != 0]                  # (not a padding tap)
        x[row, _visible_k(d, views, row, ks)] = 0.0
    elif name == "one channel taken from the neighbouring row":
        if m < 2:
            return None
        other = row - 1
        k = _visible_k(d, views, row, [k] if k is not None else [k for k in range(kk) if x[row, k] != x[other, k]])
        x[row, k] = x[other, k]
    elif name == "the last 16-byte piece of K dropped in one row":
        row = next(r for r in list(range(row, m)) + list(range(row)) if bool((x[r, kk - 8:] != 0).any()))   # (not padding)
        x[row, kk - 8:] = 0.0
        _visible_k(d, views, row, range(kk - 8, kk))
    elif name == "a 3 x 3 corner tap read from the wrapped-around pixel":
        if d["mode"] != M.CONV3X3:
            return None
        # output pixel (0, 0) of the last image, left tap of the middle row: x = -1 is padding; the flat address
        # wraps to the last pixel of the image before (of the last image, for the only one)
        up = 2 if d["upsample2x"] else 1
        hv, wv = d["hin"] * up, d["win"] * up
        img = views["a"][:, :cin].double().reshape(d["n_img"], d["hin"], d["win"], cin)
        img = img.repeat_interleave(up, 1).repeat_interleave(up, 2).reshape(-1, cin)
        i = d["n_img"] - 1
        out_row = i * d["hout"] * d["wout"]
        assert bool((x[out_row, 3 * cin:4 * cin] == 0).all())
        x[out_row, 3 * cin:4 * cin] = img[i * hv * wv - 1]
        _visible_k(d, views, out_row, range(3 * cin, 4 * cin))
    elif name == "the temporal tap of frame -1 read from the previous video's last frame":
        if d["mode"] != M.TEMPORAL3:
            return None
        per = d["frames"] * d["hw"]
        vid = m // per - 1
        out_row = vid * per                        # frame 0, pixel 0 of the last video: the row hw before it
        a = views["a"][:, :cin].double()
        assert bool((x[out_row, :cin] == 0).all())
        x[out_row, :cin] = a[out_row - d["hw"]]
        _visible_k(d, views, out_row, range(cin))
    elif name == "the a2 tap's first channel dropped":
        if not d["a2"]:
            return None
        x[:, taps * cin] = 0.0
        _visible_k(d, views, 0, [taps * cin])
    elif name == "bias2 taken from the neighbouring row group":
        rows = d["bias2_rows"] if d["bias2_rows"] > 0 else m
        if not d["bias2"] or rows >= m:
            return None
        views = dict(views, bias2=views["bias2"].roll(1, dims=0))
    else:
        raise ValueError(name)
    return x, views


GEMM_MUTANTS = ("one (row, k) element read as zero", "one channel taken from the neighbouring row",
                "the last 16-byte piece of K dropped in one row", "a 3 x 3 corner tap read from the wrapped-around pixel",
                "the temporal tap of frame -1 read from the previous video's last frame", "the a2 tap's first channel dropped",
                "bias2 taken from the neighbouring row group")


def _gemm_cases(route, bm):
    cases = [(f"draw {i}", d) for i, d in enumerate(M.exact_draws(route, bm))]
    if (route, bm) == (0, 0):
        cases += [(name, M.exact_fixed(name)) for name in sorted(M.EXACT_FIXED)]
    return cases


@pytest.mark.parametrize("route,bm", M.ROUTES)
def test_contractions_exact_in_any_order_and_every_mutant_shows(route, bm):
    rng = random.Random(M.exact_seed(route, bm))
    seen = {name: 0 for name in GEMM_MUTANTS}
    for label, d in _gemm_cases(route, bm):
        rung, _bufs, views, ref = M.exact_case(d)
        want = ref["d"].half()
        x = M.gather_rows(d, views["a"], views.get("a2") if d["a2"] else None)
        for _ in range(2):
            got = emulate(d, views, x, rng).half()
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"route ({route}, {bm}) {label}: the order of summation shows"
        for name in GEMM_MUTANTS:
            mutant = mutate(name, d, views, x)
            if mutant is None:
                continue
            seen[name] += 1
            got = M.reference(d, mutant[1], fold_formula=True, x=mutant[0])["d"].half()
            assert not torch.equal(got.view(torch.int16), want.view(torch.int16)), \
                f"route ({route}, {bm}) {label} (rung {rung}): '{name}' changes no stored value"
    print(f"route ({route}, {bm}): mutants applied {seen}")
    assert all(seen[name] >= 1 for name in GEMM_MUTANTS[:3])


def test_every_contraction_mutant_applies_somewhere():
    seen = set()
    for route, bm in M.ROUTES:
        for _label, d in _gemm_cases(route, bm):
            seen |= {"conv"} if d["mode"] == M.CONV3X3 else {"temporal"} if d["mode"] == M.TEMPORAL3 else set()
            seen |= {"a2"} if d["a2"] else set()
            rows = d["bias2_rows"] if d["bias2_rows"] > 0 else d["m"]
            seen |= {"bias2 groups"} if d["bias2"] and rows < d["m"] else set()
    assert seen == {"conv", "temporal", "a2", "bias2 groups"}


def _linear(m, n, k, seed):
    d = M.blank()
    d.update({p: M.FAKE[p] for p in ("a", "w", "d", "zero_page")})
    d.update(mode=M.LINEAR, m=m, n=n, cin=k, lda=k, ldd=n, _off={"a": 0, "d": 0}, _seed=seed, _broken=None)
    assert M.legal(d) == (True, None)
    return d


@pytest.mark.parametrize("name,m,n,k", [("one (row, k) element read as zero", 1000, 320, 320),
                                        ("one channel taken from the neighbouring row", 2016, 1280, 1280)])
def test_the_fuzz_tolerance_lets_the_first_two_mutants_pass(name, m, n, k):
    """Gaussian operands, the descriptor fuzz's own measure and bound: the planted bug passes; on integer operands it is a
    non-zero integer (the test above).  With unit-variance activations and weights / sqrt(K) a wrong term of size e in one
    row moves that row's 64 x 64 blocks by e x 8 / sqrt(K) / 64: 7.0e-3 e at K = 320, 3.5e-3 e at K = 1,280, on top of the
    rounding floor of 2e-4.  So the fuzz sees a lost element above 0.4 and a swapped channel whose two values differ by
    more than 0.8, and nothing smaller: the element here is the one of the row nearest to 0.25 (a sixth of a Gaussian's
    values are smaller), the swapped channel the one whose two values differ by nearest to 0.5."""
    d = _linear(m, n, k, seed=17)
    _bufs, views = M.make_tensors(d)
    ref = M.reference(d, views)["d"]
    x = M.gather_rows(d, views["a"])
    clean = M.errors(ref.half(), ref)
    row = m // 2
    size = x[row].abs() if "zero" in name else (x[row] - x[row - 1]).abs()
    x_bad, views_bad = mutate(name, d, views, x, k=int((size - (0.25 if "zero" in name else 0.5)).abs().argmin()))
    assert int((x_bad != x).sum()) == 1
    bad = M.errors(M.reference(d, views_bad, x=x_bad)["d"].half(), ref)
    print(f"{name} at m={m} n={n} K={k}: global {bad[0]:.2e} worst block {bad[1]:.2e} (an exact kernel: {clean[0]:.2e} / {clean[1]:.2e})")
    assert bad[1] > 2 * clean[1], "the planted bug is not there"
    assert bad[0] <= M.TOL and bad[1] <= M.TOL, "the fuzz would have caught it"


# ------------------------------------------------------------------------------------------------ attention
def _attention_sizes():
    out = []
    for seq in P.SPATIAL_SHORT + P.SPATIAL_MID + P.SPATIAL_LONG:
        out.append(pytest.param("spatial", seq, 1, 64, id=f"spatial-{seq}"))
    for frames in P.TEMPORAL_FRAMES:
        for hw in P.TEMPORAL_HW:
            out.append(pytest.param("temporal", frames, hw, 64, id=f"temporal-{frames}x{hw}"))
    for seq, hd in P.SMALL:
        out.append(pytest.param("small", seq, 1, hd, id=f"small-{seq}x{hd}"))
    return out


def _attention_patterns(kind, n, hd, scale):
    for pattern in P.PATTERNS:
        stride = P.temporal_stride(n) if kind == "temporal" else min(hd, 64)
        yield pattern, P.make(pattern, n, hd, scale, stride=stride)
    if kind == "spatial" and n in P.SPATIAL_LONG:
        nblk = n // 256
        yield "onehot_near", P.make("onehot", n, hd, scale, pi=P.far_map(n, ()))
        yield "onehot_far", P.make("onehot", n, hd, scale, pi=P.far_map(n, (1, nblk - 2)))


@pytest.mark.parametrize("kind,n,hw,hd", _attention_sizes())
def test_attention_models_pass_and_every_mutant_breaks_a_pattern(kind, n, hw, hd):
    batch, heads = 2, 2
    scale = 0.125 if hd == 64 else hd ** -0.5
    v = P.values(batch, hw, heads, n, hd, seed=n)
    caught = {m: None for m in P.MUTANTS if P.applies(m, kind, batch, hw, heads, n)}
    for pattern, (q, k, sel) in _attention_patterns(kind, n, hd, scale):
        P.check_selection(q, k, sel, scale, kind)
        s, count = P.expected(sel, v)
        if pattern.startswith("onehot"):
            assert P.must_be_bit_equal(s, count, kind == "temporal") == 1.0
        rows = P.rows_of(q, k, v)
        bad = P.violations(P.model(kind, *rows, batch, hw, heads, n, hd, scale), s, count, kind == "temporal")
        assert not bad, f"the clean model of the {kind} kernel, {pattern}: {bad}"
        for mutant in caught:
            if caught[mutant] is None and P.violations(P.model(kind, *rows, batch, hw, heads, n, hd, scale, mutant), s, count,
                                                       kind == "temporal"):
                caught[mutant] = pattern
    print(f"{kind} n={n} hw={hw} head_dim={hd}: {caught}")
    assert all(caught.values()), f"invisible at this size: {[m for m, p in caught.items() if p is None]}"
