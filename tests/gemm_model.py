"""A model of ``sp_gemm_desc`` written from the text of include/svdpipe.h (not from csrc/gemm.hip):

* ``legal(desc)``      the header's rules as a predicate over a plain dict of descriptor fields,
* ``reference(desc, tensors)``  the documented semantics in fp64 torch on the CPU from the fp16-rounded inputs,
* ``draw(rng, gen, route, legal_only)``  a seeded generator over all fields (and, with ``legal_only=False``, near-misses
  that break one rule at a time),
* ``make_tensors`` / ``to_struct``  operands for a drawn descriptor (every operand a column slice of a wider buffer whose
  slack is NaN) and the ctypes mirror of it,
* ``exact_eligible`` / ``make_exact_tensors`` / ``exact_case`` / ``exact_draws``  the same buffers filled with small non-zero
  integers, on the first rung of a value ladder on which the fp64 reference is exactly what an fp16 store holds: a kernel
  must then match it bit for bit in any order of summation (tests/test_gemm_exact_gpu.py).

A descriptor is a dict keyed by the struct's field names; pointer fields hold an address (0 = NULL; ``draw`` hands out
aligned fake ones), keys that start with ``_`` are notes of the generator (value ranges, column offsets) and not fields.
Plain helper module: no fixtures, no tests."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

LINEAR, CONV3X3, TEMPORAL3 = 0, 1, 2
TAPS = {LINEAR: 1, CONV3X3: 9, TEMPORAL3: 3}
POINTERS = ("a", "w", "bias", "bias2", "res1", "res2", "d", "zero_page", "ln_stats", "ln_colsum", "euler_latent", "euler_out",
            "euler_eps_uncond", "euler_guidance", "workspace", "ln_out", "gn_part", "a2")
FAKE = {name: 0x10000000 * (i + 1) for i, name in enumerate(POINTERS)}       # 4 KiB aligned, distinct
SCALARS = ("lda", "mode", "cin", "n_img", "hin", "win", "hout", "wout", "stride", "upsample2x", "frames", "hw", "m", "n",
           "bias2_rows", "ldb2", "ldr1", "r1scale", "ldr2", "r2scale", "oscale", "geglu", "n_store", "ldd", "euler_ld_eps",
           "euler_sigma", "euler_sigma_next", "euler_frames", "euler_hw", "workspace_bytes", "ln_out_eps", "w_group_rows",
           "w_group_stride", "lda2", "cin2", "euler_guidance_ld")
TOL = 3e-3            # the project's fuzz tolerance (fp16 storage, fp32 accumulation): tools/fuzz_gemm.py
BLOCK = 64


def blank() -> dict:
    d = {k: 0 for k in POINTERS + SCALARS}
    d.update(oscale=1.0, r1scale=1.0, r2scale=1.0, ln_out_eps=0.0, euler_sigma=0.0, euler_sigma_next=0.0)
    return d


def nout(d) -> int:
    return d["n"] // 2 if d["geglu"] else d["n"]


def stored(d) -> int:
    return d["n_store"] if d["n_store"] > 0 else nout(d)


def ln_tiles(d) -> int:
    bn = 320 if d["n"] % 320 == 0 else 256
    return d["n"] // bn if d["n"] % bn == 0 else 0


def _conv_out(size, ups, stride):
    return ((size << (1 if ups else 0)) + 2 - 3) // stride + 1


# ------------------------------------------------------------------------------------------------ legality
# (rule name, field sp_last_error() must name, predicate that holds for a legal descriptor).  Order = the order in which a
# reader meets the rules in the header; only the first broken one is reported.
def _wide(d):        # n a multiple of 256 or 320: the ping-pong tiles' widths
    return d["n"] % 256 == 0 or d["n"] % 320 == 0


RULES = [
    ("null", "null", lambda d: d["a"] and d["w"] and d["d"] and d["zero_page"]),
    ("m_positive", "m", lambda d: d["m"] > 0),
    ("n_positive", "n", lambda d: d["n"] > 0),
    ("cin_64", "cin", lambda d: d["cin"] > 0 and d["cin"] % 64 == 0),
    ("n_64", "n", lambda d: d["n"] % 64 == 0),
    ("mode", "mode", lambda d: d["mode"] in (LINEAR, CONV3X3, TEMPORAL3)),
    ("lda_min", "lda", lambda d: d["lda"] >= d["cin"]),
    ("lda_8", "lda", lambda d: d["lda"] % 8 == 0),
    ("n_store_range", "n_store", lambda d: 0 <= d["n_store"] <= nout(d)),
    ("ldd_min", "ldd", lambda d: d["ldd"] >= stored(d)),
    ("ldd_8", "ldd", lambda d: d["ldd"] % 8 == 0 or 0 < d["n_store"] < 8),
    ("gn_part_exclusions", "gn_part", lambda d: not d["gn_part"] or not (
        d["geglu"] or d["ln_stats"] or d["ln_out"] or d["euler_out"] or d["n_store"])),
    ("gn_part_m_256", "gn_part", lambda d: not d["gn_part"] or d["m"] % 256 == 0),
    ("gn_part_n", "gn_part", lambda d: not d["gn_part"] or _wide(d)),
    ("gn_part_aligned", "gn_part", lambda d: d["gn_part"] % 16 == 0),
    ("w_group_rows_128", "w_group_rows", lambda d: d["w_group_rows"] == 0 or (d["w_group_rows"] > 0 and d["w_group_rows"] % 128 == 0)),
    ("w_group_stride", "w_group_stride", lambda d: d["w_group_rows"] == 0 or (d["w_group_stride"] > 0 and d["w_group_stride"] % 8 == 0)),
    ("w_group_exclusions", "w_group_rows", lambda d: d["w_group_rows"] == 0 or (
        d["mode"] == LINEAR and not d["geglu"] and not d["euler_out"] and not d["ln_stats"] and not d["ln_colsum"])),
    ("w_group_n", "w_group_rows", lambda d: d["w_group_rows"] == 0 or _wide(d)),
    ("w_group_tile_gn_part", "w_group_rows", lambda d: not (d["w_group_rows"] and d["gn_part"]) or d["w_group_rows"] % 256 == 0),
    ("w_group_tile_ln_out", "w_group_rows", lambda d: not (d["w_group_rows"] and d["ln_out"]) or
     d["w_group_rows"] % 256 == 0 or d["w_group_rows"] % 192 == 0),
    ("w_group_tile_128", "w_group_rows", lambda d: d["w_group_rows"] == 0 or d["w_group_rows"] % 256 == 0 or
     d["w_group_rows"] % 192 == 0 or d["n"] % 256 == 0),
    ("ln_out_tiles", "ln_out", lambda d: not d["ln_out"] or 1 <= ln_tiles(d) <= 4),
    ("ln_out_exclusions", "ln_out", lambda d: not d["ln_out"] or not (d["geglu"] or d["n_store"] or d["euler_out"])),
    ("ln_out_eps", "ln_out", lambda d: not d["ln_out"] or d["ln_out_eps"] > 0),
    ("ln_out_workspace", "workspace", lambda d: not d["ln_out"] or ln_tiles(d) <= 1 or (
        d["workspace"] and d["workspace"] % 8 == 0 and d["workspace_bytes"] >= d["m"] * ln_tiles(d) * 8)),
    ("euler_conv_out", "euler", lambda d: not d["euler_out"] or (
        d["euler_latent"] and d["n"] == 64 and d["n_store"] == 4 and not d["geglu"] and not d["res1"] and not d["res2"]
        and d["oscale"] == 1.0)),
    ("euler_geometry", "euler", lambda d: not d["euler_out"] or (
        d["euler_frames"] > 0 and d["euler_hw"] > 0 and d["m"] % (d["euler_frames"] * d["euler_hw"]) == 0 and d["euler_sigma"] > 0)),
    ("euler_guidance", "euler", lambda d: not (d["euler_out"] and d["euler_eps_uncond"]) or (
        d["euler_guidance"] and d["euler_ld_eps"] >= 4 and d["euler_ld_eps"] % 4 == 0)),
    ("euler_guidance_ld", "euler_guidance_ld", lambda d: not d["euler_out"] or d["euler_guidance_ld"] == 0 or
     d["euler_guidance_ld"] >= d["euler_frames"]),
    ("ln_stats_needs", "ln_stats", lambda d: not d["ln_stats"] or (d["ln_colsum"] and d["mode"] == LINEAR and not d["bias2"])),
    ("ln_colsum_alone", "ln_colsum", lambda d: not d["ln_colsum"] or d["ln_stats"]),
    ("a2_cin2", "cin2", lambda d: not d["a2"] or (d["cin2"] > 0 and d["cin2"] % 64 == 0)),
    ("a2_lda2", "lda2", lambda d: not d["a2"] or (d["lda2"] >= d["cin2"] and d["lda2"] % 8 == 0)),
    ("a2_exclusions", "a2", lambda d: not d["a2"] or not (
        d["geglu"] or d["ln_stats"] or d["ln_out"] or d["euler_out"] or d["n_store"] or d["w_group_rows"])),
    ("a2_n", "a2", lambda d: not d["a2"] or _wide(d)),
    ("a2_gn_part_residuals", "a2", lambda d: not (d["a2"] and d["gn_part"]) or not (d["res1"] or d["res2"])),
    ("bias2_rows", "bias2_rows", lambda d: not d["bias2"] or d["bias2_rows"] >= 0),
    ("ldb2", "ldb2", lambda d: not d["bias2"] or d["ldb2"] == 0 or (d["ldb2"] >= d["n"] and d["ldb2"] % 4 == 0)),
    ("ldr1", "ldr1", lambda d: not d["res1"] or (d["ldr1"] >= stored(d) and d["ldr1"] % 8 == 0)),
    ("ldr2", "ldr2", lambda d: not d["res2"] or (d["ldr2"] >= stored(d) and d["ldr2"] % 8 == 0)),
    ("conv_stride", "stride", lambda d: d["mode"] != CONV3X3 or d["stride"] in (1, 2)),
    ("conv_positive", "n_img", lambda d: d["mode"] != CONV3X3 or min(d["n_img"], d["hin"], d["win"], d["hout"], d["wout"]) > 0),
    ("conv_output", "hout", lambda d: d["mode"] != CONV3X3 or d["stride"] not in (1, 2) or (
        d["hout"] == _conv_out(d["hin"], d["upsample2x"], d["stride"]) and d["wout"] == _conv_out(d["win"], d["upsample2x"], d["stride"]))),
    ("conv_m", "n_img*hout*wout", lambda d: d["mode"] != CONV3X3 or d["m"] == d["n_img"] * d["hout"] * d["wout"]),
    ("temporal_geometry", "frames", lambda d: d["mode"] != TEMPORAL3 or (
        d["frames"] > 0 and d["hw"] > 0 and d["m"] % (d["frames"] * d["hw"]) == 0)),
    ("geglu_n_128", "geglu", lambda d: not d["geglu"] or d["n"] % 128 == 0),
]
RULE_NAMES = [r[0] for r in RULES]


def broken_rules(desc) -> list:
    out = []
    for name, _field, ok in RULES:
        try:
            if not ok(desc):
                out.append(name)
        except ZeroDivisionError:        # a zero geometry field: the rule that asks for positive ones reports it
            pass
    return out


def legal(desc):
    """(True, None), or (False, field): the field the first broken rule is about."""
    for name in broken_rules(desc):
        return False, RULES[RULE_NAMES.index(name)][1]
    return True, None


# ------------------------------------------------------------------------------------------------ reference
def gather_rows(d, a, a2=None):
    """The [m][K] operand matrix the header describes, from the A rows (fp64)."""
    m, cin, mode = d["m"], d["cin"], d["mode"]
    a = a[:, :cin].double()
    if mode == LINEAR:
        x = a[:m]
    elif mode == CONV3X3:
        img = a[:d["n_img"] * d["hin"] * d["win"]].reshape(d["n_img"], d["hin"], d["win"], cin)
        if d["upsample2x"]:
            img = img.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        hv, wv, s = img.shape[1], img.shape[2], d["stride"]
        pad = torch.zeros(d["n_img"], hv + 2, wv + 2, cin, dtype=torch.float64)
        pad[:, 1:hv + 1, 1:wv + 1] = img
        taps = [pad[:, ky:ky + s * (d["hout"] - 1) + 1:s, kx:kx + s * (d["wout"] - 1) + 1:s].reshape(m, cin)
                for ky in range(3) for kx in range(3)]
        x = torch.cat(taps, dim=1)
    else:
        fr, hw = d["frames"], d["hw"]
        v = a[:m].reshape(m // (fr * hw), fr, hw, cin)
        pad = torch.zeros(v.shape[0], fr + 2, hw, cin, dtype=torch.float64)
        pad[:, 1:fr + 1] = v                     # frames -1 and `frames` of EVERY video are zeros
        x = torch.cat([pad[:, t:t + fr].reshape(m, cin) for t in range(3)], dim=1)
    if a2 is not None:
        x = torch.cat([x, a2[:m, :d["cin2"]].double()], dim=1)
    return x


def row_stats(x, eps):
    """(mean, 1/sqrt(var + eps)) of every row, fp64 [rows][2]."""
    x = x.double()
    return torch.stack([x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + eps)], dim=1)


def half_tile_sums(v):
    """(sum, sum of squares) per 128-row half of every 256-row tile and column: fp64 [m/256][2][n][2]."""
    m, n = v.shape
    t = v.double().reshape(m // 256, 2, 128, n)
    return torch.stack([t.sum(2), (t * t).sum(2)], dim=-1)


def euler_update(d, eps16, latent, uncond=None, guidance=None):
    """The Euler tail: eps16 fp16 [m][>=4] (the rows d would have received), latent fp16 (B,4,F,hw) -> fp64 (B,4,F,hw)."""
    fr, hw = d["euler_frames"], d["euler_hw"]
    b = d["m"] // (fr * hw)
    e = eps16[:, :4].half()
    if uncond is not None:
        ld = d["euler_guidance_ld"]
        g = guidance.float()
        g = (g[:fr].repeat(b) if ld == 0 else torch.cat([g[i * ld:i * ld + fr] for i in range(b)])).half()
        g = g.repeat_interleave(hw)[:, None]
        u = uncond[:, :4].half()
        diff = (e.float() - u.float()).half()          # evaluated in fp16, one rounding per operation
        prod = (g.float() * diff.float()).half()
        e = (u.float() + prod.float()).half()
    e = e.double().reshape(b, fr, hw, 4).permute(0, 3, 1, 2)
    sigma = float(torch.tensor(d["euler_sigma"], dtype=torch.float32))
    sigma_next = float(torch.tensor(d["euler_sigma_next"], dtype=torch.float32))
    x = latent.double().reshape(b, 4, fr, hw)
    x0 = e * (-sigma / math.sqrt(sigma * sigma + 1.0)) + x / (sigma * sigma + 1.0)
    return x + (x - x0) / sigma * (sigma_next - sigma)


def reference(d, t, fold_formula=False, x=None) -> dict:
    """fp64 results of a legal descriptor: ``d`` [m][stored columns] before the rounding to fp16, and the side outputs the
    descriptor asks for (``ln_out``, ``gn_part``, ``euler_out``).  ``t``: CPU tensors by field name, each the view the
    pointer addresses (first row / column = the pointer), weights [groups][n][K].  ``fold_formula``: a folded LayerNorm as
    the header writes it from its two inputs, ``rstd[m] * (acc - mean[m] * colsum[n])``, whatever ``ln_stats`` and
    ``ln_colsum`` hold (the exact operands hand it integers), not as ``F.layer_norm`` of the rows.  ``x``: the [m][K] operand
    matrix in place of ``gather_rows`` (tests/test_exact_patterns_cpu.py plants its mutants there)."""
    m, n = d["m"], d["n"]
    if x is None:
        x = gather_rows(d, t["a"], t.get("a2") if d["a2"] else None)
    if d["ln_stats"] and not fold_formula:
        x = F.layer_norm(x, (d["cin"],), eps=d["_ln_eps"])
    w = t["w"].double()
    if d["w_group_rows"]:
        r = d["w_group_rows"]
        acc = torch.cat([x[g * r:(g + 1) * r] @ w[g].t() for g in range((m + r - 1) // r)], dim=0)
    else:
        acc = x @ w[0].t()
    if d["ln_stats"] and fold_formula:
        st = t["ln_stats"].double()
        acc = st[:m, 1:2] * (acc - st[:m, 0:1] * t["ln_colsum"].double())
    return epilogue(d, t, acc)


def epilogue(d, t, acc) -> dict:
    """What ``reference`` does behind the contraction (and the fold): fp64 ``acc`` [m][n] -> its result dict."""
    m, n = d["m"], d["n"]
    if d["bias"]:
        acc = acc + t["bias"].double()
    if d["bias2"]:
        rows = d["bias2_rows"] if d["bias2_rows"] > 0 else m
        acc = acc + t["bias2"][:, :n].double()[torch.arange(m) // rows]
    if d["geglu"]:
        q = torch.arange(n // 2)
        val = 32 * (q // 16) + q % 16
        acc = acc[:, val] * F.gelu(acc[:, val + 16])
    v = (d["oscale"] * acc)[:, :stored(d)]
    pre = v
    if d["res1"]:
        v = v + d["r1scale"] * t["res1"][:m, :v.shape[1]].double()
    if d["res2"]:
        v = v + d["r2scale"] * t["res2"][:m, :v.shape[1]].double()
    out = {"d": v}
    if d["ln_out"]:
        out["ln_out"] = row_stats(v.half(), d["ln_out_eps"])
    if d["gn_part"]:
        out["gn_part"] = half_tile_sums(v.half() if (d["res1"] or d["res2"]) else pre)
    if d["euler_out"]:
        out["euler_out"] = euler_update(d, v.half(), t["euler_latent"], t.get("euler_eps_uncond") if d["euler_eps_uncond"] else None,
                                        t.get("euler_guidance"))
    return out


def errors(got, ref):
    """(global relative L2, worst 64 x 64 block): a block's error is ||got - ref||_block / (rms(ref) * sqrt(elements of the
    block)), so every block is held to what the whole matrix is held to."""
    got, ref = got.double(), ref.double()
    diff2 = (got - ref) ** 2
    tot = float(ref.pow(2).sum())
    glob = math.sqrt(float(diff2.sum()) / max(tot, 1e-300))
    rms2 = max(tot / ref.numel(), 1e-300)
    rows, cols = ref.shape
    pr, pc = (-rows) % BLOCK, (-cols) % BLOCK
    ones = torch.ones_like(diff2)
    s = F.pad(diff2, (0, pc, 0, pr)).reshape((rows + pr) // BLOCK, BLOCK, (cols + pc) // BLOCK, BLOCK).sum((1, 3))
    c = F.pad(ones, (0, pc, 0, pr)).reshape((rows + pr) // BLOCK, BLOCK, (cols + pc) // BLOCK, BLOCK).sum((1, 3))
    return glob, math.sqrt(float((s / (c * rms2)).max()))


# ------------------------------------------------------------------------------------------------ generator
OPTIONS = ("bias", "bias2", "res1", "res2", "oscale", "geglu", "n_store", "ln_stats", "ln_out", "w_group", "gn_part", "a2",
           "euler", "workspace")
_P = dict(bias=0.7, bias2=0.4, res1=0.5, res2=0.3, oscale=0.4, geglu=0.25, n_store=0.3, ln_stats=0.5, ln_out=0.5, w_group=0.6,
          gn_part=0.5, a2=0.45, euler=0.3, workspace=0.4)
INCOMPATIBLE = {frozenset(p) for p in [
    ("geglu", "ln_out"), ("geglu", "w_group"), ("geglu", "gn_part"), ("geglu", "a2"), ("geglu", "euler"),
    ("n_store", "ln_out"), ("n_store", "gn_part"), ("n_store", "a2"),
    ("ln_stats", "bias2"), ("ln_stats", "w_group"), ("ln_stats", "gn_part"), ("ln_stats", "a2"),
    ("ln_out", "gn_part"), ("ln_out", "a2"), ("ln_out", "euler"),
    ("w_group", "a2"), ("w_group", "euler"), ("gn_part", "euler"), ("a2", "euler"),
    ("euler", "res1"), ("euler", "res2"), ("euler", "oscale")]}
LINEAR_ONLY = ("ln_stats", "w_group")
_GENERIC = ("bias", "bias2", "res1", "res2", "oscale", "workspace")


def compatible(a, b) -> bool:
    return a != b and frozenset((a, b)) not in INCOMPATIBLE


def options_of(d) -> set:
    """Which options a descriptor exercises (for the coverage test)."""
    o = {k for k in ("bias", "bias2", "res1", "res2", "geglu", "ln_stats", "ln_out", "gn_part", "a2", "workspace") if d[k]}
    if d["oscale"] != 1.0:
        o.add("oscale")
    if d["n_store"]:
        o.add("n_store")
    if d["w_group_rows"]:
        o.add("w_group")
    if d["euler_out"]:
        o.add("euler")
    return o


def traits_of(d) -> set:
    t = set()
    if d["lda"] > d["cin"]:
        t.add("slack_lda")
    # (a linear contraction knows a batch only through its per-item rows: bias2 rows or weight groups)
    per_item = d["w_group_rows"] or (d["bias2_rows"] if d["bias2"] else 0)
    batch = {LINEAR: 2 if 0 < per_item < d["m"] else 1, CONV3X3: d["n_img"],
             TEMPORAL3: d["m"] // max(1, d["frames"] * d["hw"])}[d["mode"]]
    if batch > 1:
        t.add("batch")
    if d["m"] % 64:
        t.add("ragged_m")
    return t


def _slack(rng, width, unit=8, limit=None):
    """(row pitch, column offset) of a `width`-column slice of a wider buffer; half the time no slack at all."""
    if rng.random() < 0.4:
        return width, 0
    off = unit * rng.choice([0, 1, 2, 5])
    ld = off + width + unit * rng.choice([0, 1, 3, 8])
    if limit is not None and ld > limit:
        return width, 0
    return ld, off


def _draw_legal(rng, route, small):
    kind, bm = route
    d = blank()
    mode = rng.choice([LINEAR, LINEAR, CONV3X3, TEMPORAL3])
    if kind == 3 and rng.random() < 0.6:
        mode = LINEAR
    opts = []
    special = [o for o in OPTIONS if o not in _GENERIC]
    # (the options with many exclusions are tried first, or the common ones would always be there before them)
    for o in rng.sample(special, len(special)) + rng.sample(_GENERIC, len(_GENERIC)):
        if rng.random() < _P[o] and all(compatible(o, p) for p in opts) and not (o in LINEAR_ONLY and mode != LINEAR):
            opts.append(o)
    # forced routes: about half the draws stay clear of the options that override the route (and of what the route's
    # family does not serve), so that the family itself is exercised
    friendly = kind != 0 and rng.random() < 0.55
    if friendly:
        drop = {"gn_part", "a2", "ln_out", "w_group"} | ({"euler"} if kind != 1 else set()) | ({"n_store"} if kind == 3 else set())
        opts = [o for o in opts if o not in drop]
        if kind == 3:
            mode = LINEAR
            if bm in (128, -192):
                opts = [o for o in opts if o != "geglu"]
    if kind == 4 and "workspace" not in opts:
        opts.append("workspace")
    if "euler" in opts and "n_store" not in opts:
        opts.append("n_store")
    if "euler" in opts and mode == LINEAR and "bias2" not in opts and "ln_stats" not in opts:
        opts.append("ln_stats")                      # (two rare options: their pair would hardly ever be drawn otherwise)
    has = lambda o: o in opts   # noqa: E731
    # ---- widths
    if has("euler"):
        n = 64
    elif has("ln_out"):
        n = rng.choice([256, 320, 512, 640, 960, 1024, 1280])
    elif has("gn_part") or has("a2") or has("w_group"):
        n = rng.choice([256, 320, 512, 640, 1280])
    elif has("geglu"):
        n = rng.choice([128, 256, 512, 640, 1280, 2560])
    else:
        n = rng.choice([64, 128, 192, 256, 320, 512, 640, 960, 1280, 1920, 2560])
    if kind == 4 and n % 256 and not has("euler") and (friendly or rng.random() < 0.8):
        n = rng.choice([256, 512, 1280])
    if friendly and kind == 3:
        n = rng.choice({128: [320, 640, 960, 1280], -192: [192, 960, 1920]}.get(bm, [256, 512, 1280, 2560]))
    if friendly and kind == 2 and (not _wide({"n": n}) or (bm == 128 and n % 256)):
        n = rng.choice([256, 512, 1280] if bm == 128 else [256, 320, 640, 1280])
    if has("geglu") and n % 128:
        n = rng.choice([256, 512, 1280])
    cin = rng.choice([64, 128, 192, 320, 640] if not small else [64, 128, 192, 320])
    if kind in (3, 4) and mode == LINEAR and (friendly or rng.random() < 0.8):
        cin = rng.choice([320, 640] if small else [320, 640, 1280])
    if small:
        n = min(n, 1280)
    taps = TAPS[mode]
    cin2 = rng.choice([64, 128, 320]) if has("a2") else 0
    k = taps * cin + cin2
    cap = 1024 if small else int((2e10 if rng.random() < 0.08 else 2.5e9) // (n * k))
    need256 = has("gn_part")
    # ---- rows
    if mode == LINEAR:
        if has("w_group"):
            cands = [256, 512] if need256 else [128, 256, 384, 512, 640, 768]
            if has("ln_out"):
                cands = [c for c in cands if c % 256 == 0 or c % 192 == 0]
            if n % 256:
                cands = [c for c in cands if c % 256 == 0 or c % 192 == 0]
            rows = rng.choice(cands)
            groups = rng.choice([1, 2, 3, 5])
            while groups > 1 and groups * rows > max(cap, rows):
                groups -= 1
            m = groups * rows
            if not need256 and rng.random() < 0.3 and m > 40:
                m -= rng.choice([1, 37])                       # the last group may be short
            d["w_group_rows"], d["_groups"] = rows, groups
        elif need256:
            m = 256 * rng.choice([1, 2, 3, 4, 7, 16, 40])
        elif has("euler"):
            m = 0
        else:
            m = rng.choice([1, 7, 64, 255, 256, 257, 1000, 2560, 2561, 3000, 4097, 6001] if kind != 4 else
                           [1, 7, 255, 256, 257, 1000, 2016, 2560])
            if kind == 3 and rng.random() < 0.6:
                m = rng.choice([12000, 20001, 33000, 48000])
            if small:
                m = rng.choice([1, 7, 64, 255, 256, 257, 1000, 1024])
        if has("euler"):
            b, fr, hw = rng.choice([1, 2, 3]), rng.choice([2, 3, 5]), rng.choice([24, 60, 128])
            if small:
                b, hw = min(b, 2), min(hw, 60)
            m = b * fr * hw
            d["euler_frames"], d["euler_hw"] = fr, hw
        while m > cap and m > 256:
            m = (m // 2) if not need256 and not has("w_group") else max(256, (m // 512) * 256)
            if has("w_group"):
                break
    elif mode == CONV3X3:
        stride, ups = rng.choice([(1, 0), (1, 0), (2, 0), (1, 1)])
        if need256:
            stride, ups = 1, 0
            hin, win = rng.choice([(16, 16), (8, 32), (32, 8), (16, 32), (32, 32)])
        else:
            hin, win = rng.choice([3, 8, 17, 24] if not small else [3, 8, 17]), rng.choice([4, 9, 16, 40] if not small else [4, 9, 16])
            if ups and small:
                hin, win = min(hin, 16), min(win, 16)
        n_img = rng.choice([1, 2, 3, 5])
        hout, wout = _conv_out(hin, ups, stride), _conv_out(win, ups, stride)
        while n_img > 1 and n_img * hout * wout > cap:
            n_img -= 1
        m = n_img * hout * wout
        d.update(n_img=n_img, hin=hin, win=win, hout=hout, wout=wout, stride=stride, upsample2x=ups)
        if has("euler"):
            d["euler_frames"] = n_img if rng.random() < 0.5 else 1
            d["euler_hw"] = hout * wout
    else:
        batch = rng.choice([1, 2, 2, 3])
        if need256:
            frames, hw = rng.choice([(2, 128), (3, 256), (4, 64), (5, 256), (14, 128)])
            if (batch * frames * hw) % 256:
                batch = 2
        else:
            frames, hw = rng.choice([2, 3, 5, 14]), rng.choice([5, 33, 64, 150])
        if small and frames * hw > 1024:
            frames, hw = (2, 128) if need256 else (3, 64)
        while batch > 1 and batch * frames * hw > cap:
            batch -= 1
        if need256 and (batch * frames * hw) % 256:
            frames, hw = 2, 128
        m = batch * frames * hw
        d.update(frames=frames, hw=hw)
        if has("euler"):
            d["euler_frames"], d["euler_hw"] = frames, hw
    d.update(mode=mode, m=m, n=n, cin=cin)
    for p in ("a", "w", "d", "zero_page"):
        d[p] = FAKE[p]
    lim = 2560 if small else None
    d["lda"], off_a = _slack(rng, cin, limit=lim)
    offs = {"a": off_a}
    if has("geglu"):
        d["geglu"] = 1
    no = nout(d)
    if has("n_store"):
        d["n_store"] = 4 if has("euler") else rng.choice([3, 4, rng.randrange(1, no + 1), rng.randrange(1, no + 1)])
    st = stored(d)
    if 0 < d["n_store"] < 8 and rng.random() < 0.6:         # any pitch with fewer than 8 stored columns: rows of 4 (conv_out)
        d["ldd"], offs["d"] = st + rng.choice([0, 1, 3]), 0
    else:
        d["ldd"], offs["d"] = _slack(rng, (st + 7) // 8 * 8, limit=lim)
    if has("bias"):
        d["bias"] = FAKE["bias"]
    if has("bias2"):
        d["bias2"] = FAKE["bias2"]
        if has("w_group"):
            d["bias2_rows"] = d["w_group_rows"]
        else:
            per = {LINEAR: m, CONV3X3: d["hout"] * d["wout"], TEMPORAL3: d["frames"] * d["hw"]}[mode]
            d["bias2_rows"] = rng.choice([0, per, per, 256, 768, max(1, m // 2)] + ([1, 3] if m <= 4096 else []))
        ld, off = _slack(rng, n, unit=4, limit=lim)
        d["ldb2"], offs["bias2"] = (0, 0) if (ld == n and rng.random() < 0.5) else (ld, off)
    if has("oscale"):
        d["oscale"] = rng.choice([0.5, 2.0, 0.125])
    for r, sc in (("res1", "r1scale"), ("res2", "r2scale")):
        if has(r) and not (has("a2") and has("gn_part")):
            d[r], d[sc] = FAKE[r], rng.choice([1.0, 0.5, -0.25, 0.75])
            d["ld" + r[0] + r[-1]], offs[r] = _slack(rng, (st + 7) // 8 * 8 if d["n_store"] else no, limit=lim)
    if has("ln_stats"):
        d["ln_stats"], d["ln_colsum"], d["_ln_eps"] = FAKE["ln_stats"], FAKE["ln_colsum"], 1e-5
    if has("w_group"):
        d["w_group_stride"] = n * k + 8 * rng.choice([0, 0, 4])
    if has("a2"):
        d["a2"], d["cin2"] = FAKE["a2"], cin2
        d["lda2"], offs["a2"] = _slack(rng, cin2, limit=lim)
    if has("gn_part"):
        d["gn_part"] = FAKE["gn_part"]
    ws_bytes = 0
    if has("ln_out"):
        d["ln_out"], d["ln_out_eps"] = FAKE["ln_out"], rng.choice([1e-5, 1e-6])
        if ln_tiles(d) > 1:
            ws_bytes = m * ln_tiles(d) * 8
    if has("workspace") or ws_bytes:
        d["workspace"] = FAKE["workspace"]
        d["workspace_bytes"] = max(ws_bytes, 64)          # (the GPU fuzz widens it to what sp_gemm_workspace_bytes asks for)
    if has("euler"):
        d["euler_latent"], d["euler_out"] = FAKE["euler_latent"], FAKE["euler_out"]
        d["euler_sigma"] = rng.choice([0.5, 3.25, 31.5, 700.0])
        d["euler_sigma_next"] = d["euler_sigma"] * rng.choice([0.0, 0.6, 0.9])
        if rng.random() < 0.6:
            d["euler_eps_uncond"], d["euler_guidance"] = FAKE["euler_eps_uncond"], FAKE["euler_guidance"]
            d["euler_ld_eps"] = rng.choice([4, 8, 64])
            d["euler_guidance_ld"] = rng.choice([0, d["euler_frames"], d["euler_frames"] + 3])
    d["_off"] = offs
    return d


# One near-miss per rule: takes a legal descriptor and breaks that rule (returns False where the descriptor has no handle
# for it, e.g. no residual whose pitch could be too small).
def _need(d, *fields):
    return all(d[f] for f in fields)


def _set(desc, **kw):
    desc.update(kw)
    return True


MUTATIONS = {
    "null": lambda d, r: _set(d, **{r.choice(["a", "w", "d", "zero_page"]): 0}),
    "m_positive": lambda d, r: _set(d, m=r.choice([0, -5])),
    "n_positive": lambda d, r: _set(d, n=r.choice([0, -64])),
    "cin_64": lambda d, r: _set(d, cin=r.choice([0, d["cin"] + 8, d["cin"] - 32, -64])),
    "n_64": lambda d, r: _set(d, n=d["n"] + r.choice([8, 32, 16])),
    "mode": lambda d, r: _set(d, mode=r.choice([-1, 3, 7])),
    "lda_min": lambda d, r: _set(d, lda=d["cin"] - 8 * r.choice([1, 2, 8])),
    "lda_8": lambda d, r: _set(d, lda=d["lda"] + r.choice([1, 4, 7])),
    "n_store_range": lambda d, r: not d["euler_out"] and _set(d, n_store=r.choice([-3, -1, nout(d) + 1, nout(d) + 80])),
    "ldd_min": lambda d, r: _set(d, ldd=r.choice([8, stored(d) - 8, 0, -8]) if stored(d) > 8 else stored(d) - 1),
    "ldd_8": lambda d, r: not 0 < d["n_store"] < 8 and _set(d, ldd=d["ldd"] + r.choice([1, 4, 6])),
    "gn_part_exclusions": lambda d, r: _need(d, "gn_part") and _set(d, **r.choice([dict(n_store=8), dict(ln_out=FAKE["ln_out"], ln_out_eps=1e-5,
                                                                                                        workspace=FAKE["workspace"], workspace_bytes=1 << 20)])),
    "gn_part_m_256": lambda d, r: _need(d, "gn_part") and d["mode"] == LINEAR and not d["w_group_rows"] and _set(d, m=d["m"] + r.choice([-128, -1, -64])),
    "gn_part_n": lambda d, r: _need(d, "gn_part") and not d["w_group_rows"] and not d["a2"] and _set(d, n=r.choice([64, 128, 192, 384]), ldd=2560),
    "gn_part_aligned": lambda d, r: _need(d, "gn_part") and _set(d, gn_part=d["gn_part"] + r.choice([4, 8, 12])),
    "w_group_rows_128": lambda d, r: _need(d, "w_group_rows") and _set(d, w_group_rows=r.choice([320, 64, 200, -128])),
    "w_group_stride": lambda d, r: _need(d, "w_group_rows") and _set(d, w_group_stride=r.choice([0, -8, d["w_group_stride"] + 4])),
    "w_group_exclusions": lambda d, r: _need(d, "w_group_rows") and not d["bias2"] and _set(d, ln_stats=FAKE["ln_stats"], ln_colsum=FAKE["ln_colsum"]),
    "w_group_n": lambda d, r: _need(d, "w_group_rows") and not d["gn_part"] and not d["ln_out"] and _set(d, n=r.choice([64, 128, 192, 384]), ldd=2560),
    "w_group_tile_gn_part": lambda d, r: _need(d, "w_group_rows", "gn_part") and d["n"] % 256 == 0 and _set(d, w_group_rows=r.choice([128, 384, 640])),
    "w_group_tile_ln_out": lambda d, r: _need(d, "w_group_rows", "ln_out") and d["n"] % 256 == 0 and _set(d, w_group_rows=r.choice([128, 640])),
    "w_group_tile_128": lambda d, r: _need(d, "w_group_rows") and not d["gn_part"] and not d["ln_out"] and d["n"] % 256 != 0 and _set(
        d, w_group_rows=r.choice([128, 640])),
    "ln_out_tiles": lambda d, r: _need(d, "ln_out") and not d["w_group_rows"] and _set(d, n=r.choice([128, 192, 1536, 1920, 2560]), ldd=2560, ldr1=2560, ldr2=2560,
                                                                                      workspace=FAKE["workspace"], workspace_bytes=1 << 24),
    "ln_out_exclusions": lambda d, r: _need(d, "ln_out") and _set(d, n_store=r.choice([8, 100])),
    "ln_out_eps": lambda d, r: _need(d, "ln_out") and _set(d, ln_out_eps=r.choice([0.0, -1e-5])),
    "ln_out_workspace": lambda d, r: _need(d, "ln_out") and ln_tiles(d) > 1 and _set(d, **r.choice([
        dict(workspace=0), dict(workspace=d["workspace"] + 4), dict(workspace_bytes=d["m"] * ln_tiles(d) * 8 - 8)])),
    "euler_conv_out": lambda d, r: _need(d, "euler_out") and _set(d, **r.choice([dict(euler_latent=0), dict(oscale=0.5), dict(n_store=8),
                                                                                  dict(res1=FAKE["res1"], ldr1=64)])),
    "euler_geometry": lambda d, r: _need(d, "euler_out") and _set(d, **r.choice([dict(euler_frames=0), dict(euler_hw=d["euler_hw"] * 7 + 1 if d["m"] > 1 else 2),
                                                                                  dict(euler_sigma=0.0), dict(euler_sigma=-1.0)])),
    "euler_guidance": lambda d, r: _need(d, "euler_out", "euler_eps_uncond") and _set(d, **r.choice([dict(euler_guidance=0), dict(euler_ld_eps=0),
                                                                                                     dict(euler_ld_eps=6)])),
    "euler_guidance_ld": lambda d, r: _need(d, "euler_out") and d["euler_frames"] > 1 and _set(d, euler_guidance_ld=r.choice([d["euler_frames"] - 1, -1, 1])),
    "ln_stats_needs": lambda d, r: _need(d, "ln_stats") and _set(d, **r.choice([dict(ln_colsum=0), dict(bias2=FAKE["bias2"], bias2_rows=0, ldb2=0)])),
    "ln_colsum_alone": lambda d, r: not d["ln_stats"] and _set(d, ln_colsum=FAKE["ln_colsum"]),
    "a2_cin2": lambda d, r: _need(d, "a2") and _set(d, cin2=r.choice([0, 32, d["cin2"] + 8, -64]), lda2=2560),
    "a2_lda2": lambda d, r: _need(d, "a2") and _set(d, lda2=r.choice([d["cin2"] - 8, 8, d["lda2"] + 4, 0])),
    "a2_exclusions": lambda d, r: _need(d, "a2") and _set(d, **r.choice([dict(n_store=16), dict(geglu=1, n=1280, ldd=2560, ldr1=2560, ldr2=2560)])
                                                          if not d["gn_part"] else dict(n_store=16)),
    "a2_n": lambda d, r: _need(d, "a2") and not d["gn_part"] and _set(d, n=r.choice([64, 128, 192, 384]), ldd=2560),
    "a2_gn_part_residuals": lambda d, r: _need(d, "a2", "gn_part") and _set(d, res1=FAKE["res1"], ldr1=d["n"] + 8),
    "bias2_rows": lambda d, r: _need(d, "bias2") and _set(d, bias2_rows=r.choice([-1, -256])),
    "ldb2": lambda d, r: _need(d, "bias2") and _set(d, ldb2=r.choice([8, d["n"] - 4, d["n"] + 2, -4, d["n"] // 2])),
    "ldr1": lambda d, r: _need(d, "res1") and _set(d, ldr1=r.choice([8, stored(d) - 8, d["ldr1"] + 4, 0]) if stored(d) > 8 else 0),
    "ldr2": lambda d, r: _need(d, "res2") and _set(d, ldr2=r.choice([8, stored(d) - 8, d["ldr2"] + 4, 0]) if stored(d) > 8 else 0),
    "conv_stride": lambda d, r: d["mode"] == CONV3X3 and _set(d, stride=r.choice([0, 3, -1])),
    "conv_positive": lambda d, r: d["mode"] == CONV3X3 and _set(d, **{r.choice(["n_img", "hin", "win", "hout", "wout"]): r.choice([0, -1])}),
    "conv_output": lambda d, r: d["mode"] == CONV3X3 and d["n_img"] % 2 == 0 and _set(d, hout=d["hout"] * 2, n_img=d["n_img"] // 2),
    "conv_m": lambda d, r: d["mode"] == CONV3X3 and not d["gn_part"] and not d["euler_out"] and _set(d, m=d["m"] + r.choice([-2, -1, -d["wout"]])),
    "temporal_geometry": lambda d, r: d["mode"] == TEMPORAL3 and _set(d, **r.choice([dict(frames=0), dict(hw=0), dict(hw=d["hw"] + 1, frames=d["m"] + 1)])),
    "geglu_n_128": lambda d, r: _need(d, "geglu") and not d["ln_stats"] and _set(d, n=d["n"] + 64, ldd=2560, ldr1=2560, ldr2=2560),
}


def draw(rng, gen=None, route=(0, 0), legal_only=True, small=False, rule=None):
    """One descriptor.  ``route`` = (route, bm) as in tests/test_fuzz_gpu.py shapes the draw (route 3: long linear shapes,
    route 4: few rows and a workspace).  ``legal_only=False``: more than half the draws break one rule (``_broken``
    names it), picked uniformly from RULES so that every rule is hit.  ``small``: m <= 1,024, pitches <= 2,560, images <= 32 x 32
    (descriptors that are handed to the library to be refused)."""
    name = rule if rule else None if legal_only or rng.random() < 0.42 else RULE_NAMES[rng.randrange(len(RULES))]
    for _ in range(2000):            # (a rule about a rare combination waits for a descriptor that has a handle for it)
        d = _draw_legal(rng, route, small)
        d["_seed"] = rng.randrange(1 << 30) if gen is None else int(torch.randint(1 << 30, (1,), generator=gen))
        d["_broken"] = None
        assert legal(d)[0], (legal(d), d)
        if name is None:
            return d
        trial = dict(d)
        if MUTATIONS[name](trial, rng) and name in broken_rules(trial):
            trial["_broken"] = name
            return trial
    raise AssertionError(f"rule {name} could not be broken")


# The GPU fuzz (tests/test_gemm_descriptor_fuzz_gpu.py) and the coverage test of the generator walk the same draws.
ROUTES = [(0, 0), (2, 256), (2, 192), (2, 128), (1, 0), (3, 256), (3, 192), (3, 128), (3, -192), (4, 0)]
DRAWS_PER_ROUTE = 25


def route_seed(route, bm):
    return 7000 + 10 * route + bm


def route_draws(route, bm, count=DRAWS_PER_ROUTE):
    import random
    seed = route_seed(route, bm)
    rng, gen = random.Random(seed), torch.Generator().manual_seed(seed)
    return [draw(rng, gen, (route, bm)) for _ in range(count)]


def fuzz_draws():
    for route in ROUTES:
        for d in route_draws(*route):
            yield route, d


# ------------------------------------------------------------------------------------------------ operands
def _sliced(rows, ld, off, width, fill, dtype, values):
    """A [rows][ld] buffer filled with `fill`, `values` ([rows][width]) at columns [off, off+width): (buffer, view)."""
    buf = torch.full((rows, ld), fill, dtype=dtype)
    view = buf[:, off:off + width] if off + width <= ld else buf[:, off:]
    view.copy_(values[:, :view.shape[1]])
    return buf, view


class _Gaussian:
    """The fuzz's value ranges, drawn in the order make_tensors always drew them (a seed keeps its operands)."""

    def __init__(self, d, g):
        self.d, self.g = d, g

    def a(self, rows, cin):
        a = torch.randn(rows, cin, generator=self.g)
        if self.d["ln_stats"]:
            a = a * 1.7 + 3.0 * torch.randn(rows, 1, generator=self.g)
        return a

    def w(self, groups, n, k):
        return torch.randn(groups, n, k, generator=self.g) / math.sqrt(k)

    def a2(self, rows, cin2):
        return torch.randn(rows, cin2, generator=self.g)

    def bias(self, n):
        return torch.randn(n, generator=self.g)

    def bias2(self, rows, n):
        return torch.randn(rows, n, generator=self.g)

    def res(self, rows, cols):
        return torch.randn(rows, cols, generator=self.g)

    def ln(self, a, w):
        return row_stats(a.double(), self.d["_ln_eps"]).float(), w[0].float().sum(1)


RUNGS = [(3, 2, 1), (2, 1, 1), (1, 1, 1), (1, 1, 4), (1, 1, 16), (1, 1, 64)]     # (|a| <=, |w| <=, 1 / density of W)
EXACT_LIMIT = 1 << 24


def _ints(g, shape, top):
    """Non-zero integers in [-top, top], fp32."""
    mag = torch.randint(1, top + 1, shape, generator=g)
    return (mag * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


class _Integers:
    """Non-zero integers on a rung of RUNGS.  A thinned W keeps, for every k, the columns n = off[k] mod (1 / density): every
    operand element still meets a non-zero weight in every span of 1 / density <= 64 output columns, so no term is invisible."""

    def __init__(self, d, g, rung):
        self.d, self.g = d, g
        self.amax, self.wmax, self.thin = RUNGS[rung]

    def a(self, rows, cin):
        return _ints(self.g, (rows, cin), self.amax)

    def w(self, groups, n, k):
        w = _ints(self.g, (groups, n, k), self.wmax)
        if self.thin > 1:
            off = torch.randint(0, self.thin, (groups, 1, k), generator=self.g)
            w = w * (torch.arange(n)[None, :, None] % self.thin == off)
        return w

    def a2(self, rows, cin2):
        return _ints(self.g, (rows, cin2), self.amax)

    def bias(self, n):
        return _ints(self.g, (n,), 8)

    def bias2(self, rows, n):
        return _ints(self.g, (rows, n), 8)

    def res(self, rows, cols):
        return _ints(self.g, (rows, cols), 8)

    def ln(self, a, w):
        """Integer means, power-of-two rstd, the weight's own (integer) row sums."""
        rows = a.shape[0]
        mean = torch.randint(-3, 4, (rows,), generator=self.g).float()
        rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (rows,), generator=self.g)]
        return torch.stack([mean, rstd], dim=1), w[0].float().sum(1)


def make_tensors(d, gen=None, values=None):
    """CPU operands of a legal descriptor: ``bufs`` (name -> the wide buffer, slack = NaN) and ``views`` (name -> what the
    descriptor's pointer addresses, for reference()).  Value ranges follow the existing kernel tests (unit-variance
    activations, weights / sqrt(K), folded-LayerNorm rows with a common offset of up to ~3 standard deviations);
    ``values`` (make_exact_tensors) replaces the ranges and nothing else."""
    g = gen if gen is not None else torch.Generator().manual_seed(d["_seed"])
    v = values if values is not None else _Gaussian(d, g)
    nan = float("nan")
    m, n, cin, mode = d["m"], d["n"], d["cin"], d["mode"]
    off = d["_off"]
    bufs, views = {}, {}
    rows_in = d["n_img"] * d["hin"] * d["win"] if mode == CONV3X3 else m
    a = v.a(rows_in, cin)
    bufs["a"], views["a"] = _sliced(rows_in, d["lda"], off["a"], cin, nan, torch.float16, a.half())
    k = TAPS[mode] * cin + d["cin2"]
    groups = d.get("_groups", 1) if d["w_group_rows"] else 1
    stride = d["w_group_stride"] if d["w_group_rows"] else n * k
    wbuf = torch.full((groups * stride,), nan, dtype=torch.float16)
    w = v.w(groups, n, k).half()
    for i in range(groups):
        wbuf[i * stride:i * stride + n * k] = w[i].reshape(-1)
    bufs["w"], views["w"] = wbuf, w
    if d["a2"]:
        bufs["a2"], views["a2"] = _sliced(m, d["lda2"], off["a2"], d["cin2"], nan, torch.float16, v.a2(m, d["cin2"]).half())
    if d["bias"]:
        bufs["bias"] = views["bias"] = v.bias(n)
    if d["bias2"]:
        rows = d["bias2_rows"] if d["bias2_rows"] > 0 else m
        nb = (m + rows - 1) // rows
        bufs["bias2"], views["bias2"] = _sliced(nb, d["ldb2"] or n, off.get("bias2", 0), n, nan, torch.float32, v.bias2(nb, n))
    st = stored(d)
    for r in ("res1", "res2"):
        if d[r]:
            ld = d["ld" + r[0] + r[-1]]
            bufs[r], views[r] = _sliced(m, ld, off[r], st, nan, torch.float16, v.res(m, st).half())
    if d["ln_stats"]:
        stats, colsum = v.ln(views["a"][:, :cin], w)
        bufs["ln_stats"] = views["ln_stats"] = stats
        bufs["ln_colsum"] = views["ln_colsum"] = colsum
    if d["euler_out"]:
        b = m // (d["euler_frames"] * d["euler_hw"])
        scale = max(1.0, d["euler_sigma"])
        bufs["euler_latent"] = views["euler_latent"] = (torch.randn(b, 4, d["euler_frames"], d["euler_hw"], generator=g) * scale).half()
        if d["euler_eps_uncond"]:
            ld = d["euler_ld_eps"]
            bufs["euler_eps_uncond"], views["euler_eps_uncond"] = _sliced(m, ld, 0, 4, nan, torch.float16,
                                                                          torch.randn(m, 4, generator=g).half())
            gl = d["euler_guidance_ld"]
            gs = torch.full((b * gl if gl else d["euler_frames"],), nan)
            for i in range(b if gl else 1):
                gs[i * gl:i * gl + d["euler_frames"]] = torch.linspace(1.0, 1.5 + i, d["euler_frames"])
            bufs["euler_guidance"] = views["euler_guidance"] = gs
    return bufs, views


# ------------------------------------------------------------------------------------------------ exact operands
def exact_eligible(d) -> bool:
    """Whether integer operands make the header's arithmetic exact in fp32.  Not GEGLU (a gelu) and not the Euler tail
    (non-dyadic sigmas, fp16 guidance arithmetic).  A folded LayerNorm IS: ``ln_stats`` and ``ln_colsum`` are inputs, and
    all three kernels evaluate ``(acc - mean * colsum) * rstd + bias`` in fp32 (gemm.hip, gemm_pp.hip and gemm_ps.hip
    epilogues); with integer means and column sums and a power-of-two rstd every step, fused or not, is an integer below
    2^24 times a power of two.  ``ln_out`` is a side output with its own tolerance and does not touch ``d``."""
    return not d["geglu"] and not d["euler_out"]


def make_exact_tensors(d, rung):
    """``make_tensors`` with non-zero integers on rung ``rung`` of RUNGS for A, a2 and W, integers in [-8, 8] for the biases
    and residuals, and integer / power-of-two LayerNorm statistics; buffers, offsets, NaN slack and weight groups as ever."""
    assert exact_eligible(d)
    g = torch.Generator().manual_seed(d["_seed"] + 7919 * (rung + 1))
    return make_tensors(d, g, _Integers(d, g, rung))


def exact_unit(d) -> float:
    """The grid of the stored values: the largest power of two that divides oscale and the residual scales in use."""
    def low(s):
        f = abs(float(s))
        u = 1.0
        while f != math.floor(f):
            f, u = f * 2.0, u / 2.0
        while f % 2.0 == 0.0:
            f, u = f / 2.0, u * 2.0
        return u
    return min([low(d["oscale"])] + [low(d[s]) for r, s in (("res1", "r1scale"), ("res2", "r2scale")) if d[r]])


def exact_case(d):
    """(rung, bufs, views, reference) at the first rung of RUNGS on which
    * reference(d)["d"] equals its own .half(): the stored fp16 is the integer result itself;
    * sum |a||w| (with a fold: + |mean||colsum|), the biases and the residuals stay below 2^24 for every output, so that
      every partial sum of any order is exact in fp32;
    * with gn_part, every half tile's column sum of |v| and of v^2 stays below 2^24 in units of the output grid.
    Conditions on the inputs alone.  A draw without a rung is an error of the generator."""
    k = TAPS[d["mode"]] * d["cin"] + d["cin2"]
    for rung, (amax, wmax, _thin) in enumerate(RUNGS):
        bufs, views = make_exact_tensors(d, rung)
        ref = reference(d, views, fold_formula=True)
        v = ref["d"]
        if not torch.equal(v.half().double(), v):
            continue
        terms = k * amax * wmax                                   # sum |a||w|
        if d["ln_stats"]:
            terms = 2 * (terms + 3 * k * wmax)                    # |mean| <= 3, |colsum| <= K |w|, rstd <= 2
        assert (terms + 16) * max(1.0, d["oscale"]) + 16 < EXACT_LIMIT        # + biases, residuals (each <= 8)
        if d["gn_part"]:
            u = v / exact_unit(d)
            assert torch.equal(u, u.round())
            s = half_tile_sums(u.abs())
            if float(s[..., 0].max()) >= EXACT_LIMIT or float(s[..., 1].max()) >= EXACT_LIMIT:
                continue
        return rung, bufs, views, ref
    raise AssertionError(f"no rung of the value ladder makes this draw exact: {d}")


def exact_rung(d) -> int:
    return exact_case(d)[0]


EXACT_DRAWS_PER_ROUTE = 12
EXACT_MNK = 1e9


def exact_seed(route, bm):
    return 9000 + 10 * route + bm


def exact_small(route, bm) -> bool:
    """Routes whose family serves m <= 1,024 (all but the persistent-stream ones, which want many rows)."""
    return route != 3


def stream_shaped(d, bm) -> bool:
    """A draw that a forced persistent-stream route keeps (the header's list for sp_gemm_set_route(3): plain rows, whole
    column tiles, K >= 256, every column stored, none of the options that pin the 256-row ping-pong tiles, bias2 rows that
    no tile straddles, an even m with a folded LayerNorm)."""
    bn = {128: 320, -192: 192}.get(bm, 256)
    rows = {128: 128, -192: 256}.get(bm, bm)
    return (d["mode"] == LINEAR and d["n"] % bn == 0 and d["cin"] >= 256 and not d["n_store"] and not d["gn_part"] and not d["a2"]
            and not d["ln_out"] and not d["w_group_rows"] and not (d["ln_stats"] and d["m"] % 2)
            and not (d["bias2"] and 0 < d["bias2_rows"] < d["m"] and d["bias2_rows"] % rows))


def exact_draws(route, bm, count=EXACT_DRAWS_PER_ROUTE):
    """The exact tests' own seeded series: eligible draws with m * n * K <= 1e9 (the cost is the fp64 reference).  On the
    persistent-stream routes at most 5 of the 12 are shapes that the family hands to another kernel."""
    import random
    seed = exact_seed(route, bm)
    rng, gen = random.Random(seed), torch.Generator().manual_seed(seed)
    out, other = [], 0
    while len(out) < count:
        d = draw(rng, gen, (route, bm), small=exact_small(route, bm))
        if not exact_eligible(d) or d["m"] * d["n"] * (TAPS[d["mode"]] * d["cin"] + d["cin2"]) > EXACT_MNK:
            continue
        if route == 3 and not stream_shaped(d, bm):
            other += 1
            if other > 5:
                continue
        out.append(d)
    return out


# Geometries the draws do not reach by name (every route's small-tile or ping-pong kernel takes them).
EXACT_FIXED = {
    # a 3 x 3 convolution at stride 2 over odd images: the last output row and column read pixel row hin - 1 and padding
    "conv_stride2_odd": dict(mode=CONV3X3, n_img=3, hin=7, win=5, hout=4, wout=3, stride=2, m=36, n=256, cin=64, lda=72, ldd=272,
                             _off={"a": 8, "d": 8}, _seed=101),
    # two frames of five pixels: every row is a first or a last frame, an outer tap is padding in every row
    "temporal_two_frames": dict(mode=TEMPORAL3, frames=2, hw=5, m=30, n=256, cin=128, lda=128, ldd=256, res1=FAKE["res1"], ldr1=256,
                                r1scale=0.5, _off={"a": 0, "d": 0, "res1": 0}, _seed=102),
}


def exact_fixed(name) -> dict:
    d = blank()
    d.update({p: FAKE[p] for p in ("a", "w", "d", "zero_page", "bias")})
    d.update(_broken=None, **EXACT_FIXED[name])
    assert legal(d) == (True, None) and exact_eligible(d), legal(d)
    return d


def to_struct(d, pointers=None):
    """ctypes mirror of the descriptor; ``pointers`` overrides addresses by field name."""
    from vdpp_amd import hip
    s = hip.GemmDesc()
    for name, _ctype in hip.GemmDesc._fields_:
        v = d[name]
        if pointers is not None and name in pointers:
            v = pointers[name]
        if name in POINTERS:
            v = int(v) or None
        setattr(s, name, v)
    return s
