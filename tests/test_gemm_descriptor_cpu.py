"""sp_gemm_desc held to include/svdpipe.h without a GPU (tests/gemm_model.py is the model):

* the model's fp64 reference against the obvious torch expression of every option (what makes it a yardstick),
* legality: a table of descriptors the library must refuse (SP_EINVAL, sp_last_error() names the field) and of descriptors
  the product issues that it must not, then a seeded differential run of the library against ``legal()``,
* the generator's coverage over the seeds the GPU fuzz uses, and the error an exact kernel with fp16 stores would show by the
  two measures that fuzz applies,
* the per-block measure catches a defect the global one hides.

Validation is host code: without a GPU an accepted descriptor ends in SP_ELAUNCH (-2, no device), a refused one in
SP_EINVAL (-1), nothing can launch.  With a GPU an accepted descriptor DOES launch, so there every pointer lies in the middle
of one zero-filled arena with 64 MiB on both sides, and every descriptor is checked to reach no further than that before it is
submitted (shapes here stay at m <= 1,024, pitches <= 2,560, images <= 32 x 32; the weights, n x K halves per row group, are
what needs the room)."""
import ctypes
import collections
import math
import os
import random
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_model as M  # noqa: E402

from vdpp_amd import hip  # noqa: E402
from vdpp_amd.models import weights as W  # noqa: E402

MAX_M, MAX_LD = 1024, 2560
# m x pitch x 4 bytes bounds every activation-side operand; the weights (n x K halves, times the row groups) are larger
HALF_ARENA = 64 << 20


def reach_bytes(d):
    """The furthest byte behind any of its pointers a descriptor can make the library touch."""
    m, n = max(d["m"], 0), max(d["n"], 0)
    k = M.TAPS.get(d["mode"], 1) * max(d["cin"], 0) + max(d["cin2"], 0)
    rows_in = max(m, d["n_img"] * d["hin"] * d["win"]) if d["mode"] == M.CONV3X3 else m
    groups = (m + d["w_group_rows"] - 1) // d["w_group_rows"] if d["w_group_rows"] > 0 else 1
    return max(rows_in * abs(d["lda"]) * 2, (groups * abs(d["w_group_stride"]) + n * k) * 2, m * abs(d["ldd"]) * 2 + 16,
               m * abs(d["ldr1"]) * 2 + 16, m * abs(d["ldr2"]) * 2 + 16, (m + 1) * max(abs(d["ldb2"]), n) * 4, m * abs(d["lda2"]) * 2,
               m * n * 4 + 16, d["workspace_bytes"], m * max(abs(d["euler_ld_eps"]), 4) * 2, (m + 1) * (abs(d["euler_guidance_ld"]) + 64) * 4)


def h(t):
    return t.half()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ calling the library
@pytest.fixture(scope="module")
def submit():
    """submit(desc) -> (rc, message).  Pointers: the descriptor's (aligned, fake) addresses without a GPU; with one, the same
    offsets within 4 KiB from the middle of a zero-filled device arena, and one synchronize at the end."""
    lib = hip.load()
    arena = None
    if torch.cuda.is_available():
        arena = torch.zeros(2 * HALF_ARENA, dtype=torch.uint8, device="cuda")
        mid = (arena.data_ptr() + HALF_ARENA + 4095) // 4096 * 4096

    def run(desc):
        assert desc["m"] <= MAX_M and max(desc[k] for k in ("lda", "ldd", "ldr1", "ldr2", "ldb2", "lda2")) <= MAX_LD, \
            "descriptors handed to the library here stay small"
        assert reach_bytes(desc) <= HALF_ARENA, "a descriptor that could reach outside the arena"
        ptrs = None
        if arena is not None:
            ptrs = {p: mid + (desc[p] & 4095) for p in M.POINTERS if desc[p]}
        rc = lib.sp_gemm_f16(ctypes.byref(M.to_struct(desc, ptrs)), None)
        return rc, lib.sp_last_error().decode() if rc else ""

    yield run
    if arena is not None:
        torch.cuda.synchronize()


def base(mode=M.LINEAR, m=1024, n=320, cin=320, **kw):
    d = M.blank()
    for p in ("a", "w", "d", "zero_page"):
        d[p] = M.FAKE[p]
    d.update(mode=mode, m=m, n=n, cin=cin, lda=cin)
    for k, v in kw.items():
        d[k] = M.FAKE[k] if (k in M.POINTERS and v is True) else v
    d.setdefault("_off", {})
    if "ldd" not in kw:
        d["ldd"] = (M.stored(d) + 7) // 8 * 8 if not d["n_store"] else M.stored(d)
    for r, ld in (("res1", "ldr1"), ("res2", "ldr2")):
        if d[r] and ld not in kw:
            d[ld] = (M.stored(d) + 7) // 8 * 8
    if d["a2"] and "lda2" not in kw:
        d["lda2"] = d["cin2"]
    return d


def conv(n_img, hin, win, stride=1, ups=0, **kw):
    ho, wo = M._conv_out(hin, ups, stride), M._conv_out(win, ups, stride)
    return base(M.CONV3X3, m=n_img * ho * wo, n_img=n_img, hin=hin, win=win, hout=ho, wout=wo, stride=stride, upsample2x=ups, **kw)


# The descriptors of the issue's table: each was accepted before this file existed.
ILLEGAL_TABLE = [
    ("gn_part + w_group_rows=128", base(gn_part=True, w_group_rows=128, w_group_stride=320 * 320), "w_group_rows"),
    ("gn_part + w_group_rows=384", base(m=768, gn_part=True, w_group_rows=384, w_group_stride=320 * 320), "w_group_rows"),
    ("ldd=8 with 320 stored columns", base(ldd=8), "ldd"),
    ("res1 with ldr1=8", base(res1=True, ldr1=8), "ldr1"),
    ("res2 with ldr2=8", base(res2=True, ldr2=8), "ldr2"),
    ("bias2 with ldb2=8", base(bias2=True, bias2_rows=256, ldb2=8), "ldb2"),
    ("n_store=400 > n", base(n_store=400, ldd=400), "n_store"),
    ("n_store=-3", base(n_store=-3, ldd=320), "n_store"),
    ("ln_colsum without ln_stats", base(ln_colsum=True), "ln_colsum"),
]


def legal_table():
    """What models/unet_hip.py, vae_hip.py and clip_hip.py pass to ops.gemm, at small row counts: every option, the pitches
    the product really uses (lda = a.stride(0) of a concatenation buffer, ldb2 = the whole time-embedding row, ldd = 4 for
    conv_out, residuals as halves of wider buffers)."""
    ws = dict(workspace=True, workspace_bytes=1 << 16)
    eul = dict(n=64, n_store=4, ldd=4, euler_latent=True, euler_out=True, euler_sigma=31.5, euler_sigma_next=20.25)
    t = [
        base(bias=True), base(m=1000, bias=True, res1=True), base(m=77, n=64, cin=128), base(m=1, n=1280, cin=1280, bias=True),
        base(n=960, bias=True, lda=640), base(n=1920, cin=640, lda=1280), base(n=2560, cin=320, geglu=1, bias=True, ln_stats=True, ln_colsum=True),
        base(n=960, ln_stats=True, ln_colsum=True), base(n=1280, cin=1280, bias=True, res1=True, ldr1=2560, **ws),
        base(m=1000, n=320, cin=1280, bias=True, res1=True, ln_out=True, ln_out_eps=1e-5),
        base(n=640, cin=640, bias=True, res1=True, ln_out=True, ln_out_eps=1e-5, workspace=True, workspace_bytes=1024 * 2 * 8),
        base(n=1280, cin=1280, res1=True, res2=True, r2scale=0.5, ln_out=True, ln_out_eps=1e-5, workspace=True, workspace_bytes=1024 * 4 * 8),
        base(n=256, cin=64, bias2=True, bias2_rows=1000, ln_out=True, ln_out_eps=1e-5),
        base(n=320, cin=320, bias2=True, bias2_rows=256, w_group_rows=256, w_group_stride=320 * 320),
        base(n=640, cin=640, bias2=True, bias2_rows=512, w_group_rows=512, w_group_stride=640 * 640, res1=True),
        base(n=1280, cin=1280, bias2=True, bias2_rows=128, w_group_rows=128, w_group_stride=1280 * 1280),
        base(n=320, cin=320, bias2=True, bias2_rows=384, m=768, w_group_rows=384, w_group_stride=320 * 320, ln_out=True, ln_out_eps=1e-5),
        base(n=320, cin=320, bias2=True, bias2_rows=256, w_group_rows=256, w_group_stride=320 * 320, gn_part=True),
        base(n=320, bias=True, gn_part=True), base(n=640, cin=320, bias=True, bias2=True, bias2_rows=1024, ldb2=2560, gn_part=True),
        base(n=1280, cin=128, bias=True, res1=True, res2=True, oscale=0.5, gn_part=True),
        base(n=640, cin=256, a2=True, cin2=960, bias=True), base(n=320, cin=320, a2=True, cin2=640, lda2=1280, bias=True, gn_part=True),
        base(n=320, cin=320, a2=True, cin2=64, res1=True, r1scale=0.75),
        base(n=512, cin=64, n_store=3, ldd=3, bias=True), base(n=64, cin=64, n_store=8, ldd=8), base(n=128, cin=128, n_store=13, ldd=16, res1=True, ldr1=128),
        base(n=1280, cin=320, geglu=1, n_store=600, ldd=640), base(n=256, cin=64, geglu=1, bias=True, oscale=2.0, res1=True),
        base(n=192, cin=64), base(n=1920, cin=320, oscale=0.125), base(m=257, n=64, cin=64, bias=True, bias2=True, bias2_rows=0, ldb2=0),
        base(m=600, euler_frames=5, euler_hw=60, **eul), base(m=600, euler_frames=5, euler_hw=60, euler_eps_uncond=True, euler_guidance=True, euler_ld_eps=4, **eul),
        conv(2, 16, 16, n=320, cin=64, bias=True, bias2=True, bias2_rows=256, ldb2=1280),
        conv(4, 16, 16, n=320, cin=320, bias=True, gn_part=True), conv(1, 32, 32, n=640, cin=64, lda=128, bias=True, res1=True, ldr1=1280),
        conv(3, 17, 16, stride=2, n=320, cin=320, bias=True), conv(2, 8, 8, ups=1, n=640, cin=640, bias=True, **ws),
        conv(4, 16, 16, n=320, cin=320, a2=True, cin2=640, bias=True, gn_part=True),
        conv(2, 16, 16, n=256, cin=128, a2=True, cin2=64, lda2=128, bias=True, res1=True),
        conv(1, 8, 16, n=64, cin=64, n_store=3, ldd=3, bias=True), conv(3, 8, 25, cin=320, bias=True, euler_frames=3, euler_hw=200, **eul),
        conv(2, 8, 25, cin=320, bias=True, euler_frames=2, euler_hw=200, euler_eps_uncond=True, euler_guidance=True, euler_ld_eps=4,
             euler_guidance_ld=2, **eul),
        base(M.TEMPORAL3, m=2 * 3 * 64, n=320, cin=320, frames=3, hw=64, bias=True, res1=True, r1scale=0.5, oscale=0.5),
        base(M.TEMPORAL3, m=2 * 2 * 128, n=640, cin=64, frames=2, hw=128, bias=True, gn_part=True),
        base(M.TEMPORAL3, m=14 * 64, n=1280, cin=1280, frames=14, hw=64, bias=True, bias2=True, bias2_rows=14 * 64, **ws),
        base(M.TEMPORAL3, m=2 * 256, n=320, cin=64, frames=2, hw=256, a2=True, cin2=128, bias=True),
        base(m=1024, n=1024, cin=1024, lda=1032), base(m=50, n=768, cin=768, bias=True, res1=True), base(m=514, n=2048, cin=1024, bias=True, ln_stats=True, ln_colsum=True),
    ]
    return t


# ------------------------------------------------------------------------------------------------ reference vs plain torch
def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).half()


def test_reference_linear_epilogue():
    g = torch.Generator().manual_seed(1)
    m, n, cin = 300, 128, 192
    a, w = _rand(g, m, cin + 16), _rand(g, 1, n, cin, scale=cin ** -0.5)
    b, b2 = torch.randn(n, generator=g), torch.randn(3, n + 4, generator=g)
    r1, r2 = _rand(g, m, n + 8), _rand(g, m, n)
    d = base(m=m, n=n, cin=cin, lda=cin + 16, bias=True, bias2=True, bias2_rows=128, ldb2=n + 4, res1=True, ldr1=n + 8, r1scale=-0.25,
             res2=True, r2scale=0.75, oscale=0.5, n_store=100)
    got = M.reference(d, dict(a=a, w=w, bias=b, bias2=b2, res1=r1, res2=r2))["d"]
    A, Wt = a[:, :cin].double(), w[0].double()
    want = 0.5 * (A @ Wt.t() + b.double() + b2[:, :n].double().repeat_interleave(128, 0)[:m]) - 0.25 * r1[:, :n].double() + 0.75 * r2.double()
    assert got.shape == (m, 100) and rel(got, want[:, :100]) <= 1e-12
    d0 = base(m=m, n=n, cin=cin, lda=cin + 16, bias2=True, bias2_rows=0)              # bias2_rows 0: one row for every m
    assert rel(M.reference(d0, dict(a=a, w=w, bias2=b2))["d"], A @ Wt.t() + b2[0, :n].double()) <= 1e-12


@pytest.mark.parametrize("stride,ups", [(1, 0), (2, 0), (1, 1)])
def test_reference_conv3x3_with_extra_linear_tap(stride, ups):
    g = torch.Generator().manual_seed(2)
    n_img, hin, win, cin, cin2, n = 2, 7, 10, 64, 128, 256
    x = _rand(g, n_img, cin, hin, win)
    wc, w1 = _rand(g, n, cin, 3, 3, scale=0.05), _rand(g, n, cin2, 1, 1, scale=0.1)
    d = conv(n_img, hin, win, stride=stride, ups=ups, n=n, cin=cin, a2=True, cin2=cin2, lda2=cin2 + 8)
    x2 = _rand(g, n_img, cin2, d["hout"], d["wout"])
    a = x.permute(0, 2, 3, 1).reshape(-1, cin)
    a2 = torch.cat([x2.permute(0, 2, 3, 1).reshape(-1, cin2), _rand(g, d["m"], 8)], dim=1)
    w = torch.cat([W.pack_conv3x3(wc), w1.reshape(n, cin2)], dim=1)[None]
    got = M.reference(d, dict(a=a, w=w, a2=a2))["d"]
    xin = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if ups else x.double()
    want = F.conv2d(xin, wc.double(), None, padding=1, stride=stride) + F.conv2d(x2.double(), w1.double())
    assert rel(got, want.permute(0, 2, 3, 1).reshape(d["m"], n)) <= 1e-12


def test_reference_temporal_batch_of_two():
    g = torch.Generator().manual_seed(3)
    b, fr, hw, cin, n = 2, 5, 6, 64, 128
    x = _rand(g, b, cin, fr, hw, 1)
    wt = _rand(g, n, cin, 3, 1, 1, scale=0.1)
    d = base(M.TEMPORAL3, m=b * fr * hw, n=n, cin=cin, frames=fr, hw=hw)
    a = x[..., 0].permute(0, 2, 3, 1).reshape(-1, cin)
    got = M.reference(d, dict(a=a, w=W.pack_tconv3(wt)[None]))["d"]
    want = F.conv3d(x.double(), wt.double(), None, padding=(1, 0, 0))[..., 0].permute(0, 2, 3, 1).reshape(d["m"], n)
    assert rel(got, want) <= 1e-12
    # video 1's first frame must not see video 0's last one: the two videos alone give the same rows
    for i in range(b):
        one = base(M.TEMPORAL3, m=fr * hw, n=n, cin=cin, frames=fr, hw=hw)
        alone = M.reference(one, dict(a=a[i * fr * hw:(i + 1) * fr * hw], w=W.pack_tconv3(wt)[None]))["d"]
        assert torch.equal(alone, got[i * fr * hw:(i + 1) * fr * hw])


def test_reference_folded_layernorm_geglu():
    g = torch.Generator().manual_seed(4)
    m, cin, n = 200, 128, 256
    x = (torch.randn(m, cin, generator=g) * 1.7 + 3.0 * torch.randn(m, 1, generator=g)).half()
    gamma, beta = 1.0 + 0.3 * torch.randn(cin, generator=g), 0.5 * torch.randn(cin, generator=g)
    w, b = torch.randn(n, cin, generator=g) / math.sqrt(cin), torch.randn(n, generator=g)
    wg = (w * gamma).half()                                   # the fold: gamma into the weights, beta into the bias
    bf = (w.double() @ beta.double() + b.double())
    wi, bi = W.interleave_geglu(wg, bf.float())
    d = base(m=m, n=n, cin=cin, geglu=1, bias=True, ln_stats=True, ln_colsum=True, _ln_eps=1e-5)
    got = M.reference(d, dict(a=x, w=wi[None], bias=bi))["d"]
    y = F.layer_norm(x.double(), (cin,), eps=1e-5) @ wg.double().t() + bf.float().double()
    want = y[:, :n // 2] * F.gelu(y[:, n // 2:])
    assert got.shape == (m, n // 2) and rel(got, want) <= 1e-12


def test_reference_per_group_weights():
    g = torch.Generator().manual_seed(5)
    m, cin, n, rows = 700, 64, 256, 256
    a, w = _rand(g, m, cin), _rand(g, 3, n, cin, scale=0.1)
    b2 = torch.randn(3, n, generator=g)
    d = base(m=m, n=n, cin=cin, w_group_rows=rows, w_group_stride=n * cin, bias2=True, bias2_rows=rows)
    got = M.reference(d, dict(a=a, w=w, bias2=b2))["d"]
    for i in range(3):
        sl = slice(i * rows, min(m, (i + 1) * rows))
        assert rel(got[sl], a[sl].double() @ w[i].double().t() + b2[i].double()) <= 1e-12


@pytest.mark.parametrize("residual", [False, True])
def test_reference_groupnorm_sums_and_row_statistics(residual):
    g = torch.Generator().manual_seed(6)
    m, cin, n, groups = 512, 64, 256, 32
    a, w, b = _rand(g, m, cin), _rand(g, 1, n, cin, scale=0.1), torch.randn(n, generator=g) + 3.0
    t = dict(a=a, w=w, bias=b)
    kw = {}
    if residual:
        t["res1"] = _rand(g, m, n)
        kw = dict(res1=True)
    out = M.reference(base(m=m, n=n, cin=cin, bias=True, gn_part=True, **kw), t)
    v = out["d"].half().double() if residual else out["d"]           # with residuals the sums are of the stored values
    part = out["gn_part"]
    assert part.shape == (m // 256, 2, n, 2)
    for inst, rows in ((2, 256), (1, 512), (4, 128)):                # any instance that is a whole number of 128-row halves
        s = part.reshape(inst, rows // 128, n, 2).sum(1)
        cnt = rows * (n // groups)
        mean = s[..., 0].reshape(inst, groups, -1).sum(2) / cnt
        var = s[..., 1].reshape(inst, groups, -1).sum(2) / cnt - mean * mean
        x = v.reshape(inst, rows, n).permute(0, 2, 1)
        want = F.group_norm(x, groups, eps=1e-6)
        mine = (x.reshape(inst, groups, -1) - mean[..., None]) / torch.sqrt(var[..., None] + 1e-6)
        assert rel(mine.reshape(want.shape), want) <= 1e-9           # (E[x^2] - mean^2 in fp64: cancellation costs digits)
    lo = M.reference(base(m=m, n=n, cin=cin, bias=True, ln_out=True, ln_out_eps=1e-5, **kw), t)
    x16 = lo["d"].half().double()
    st = lo["ln_out"]
    assert rel((x16 - st[:, :1]) * st[:, 1:], F.layer_norm(x16, (n,), eps=1e-5)) <= 1e-12


@pytest.mark.parametrize("guidance_ld", [None, 0, 7])
def test_reference_euler_tail_against_the_oracle_step(guidance_ld):
    from oracle.svd_step_ref import svd_step
    g = torch.Generator().manual_seed(7)
    b, fr, hh, ww, cin = 2, 5, 3, 4, 64
    hw, m = hh * ww, 2 * 5 * 12
    sigma, sigma_next = 31.5, 20.25
    lat = _rand(g, b, 4, fr, hh, ww, scale=30.0)
    a, w = _rand(g, m, cin), _rand(g, 1, 64, cin, scale=0.1)
    d = base(m=m, n=64, cin=cin, n_store=4, ldd=4, euler_latent=True, euler_out=True, euler_sigma=sigma, euler_sigma_next=sigma_next,
             euler_frames=fr, euler_hw=hw)
    t = dict(a=a, w=w, euler_latent=lat.reshape(b, 4, fr, hw))
    eps_c = (a.double() @ w[0].double().t())[:, :4].half()            # what d would have received

    def as_unet_output(rows):                                        # (B, F, 4, H, W), as the UNet returns it
        return rows.reshape(b, fr, hh, ww, 4).permute(0, 1, 4, 2, 3)

    kw = dict(sigmas=torch.tensor([sigma, sigma_next], dtype=torch.float64), timesteps=[0], image_embeddings=torch.zeros(1),
              image_latents=torch.zeros(b, 4, fr, hh, ww), added_time_ids=None)
    if guidance_ld is None:
        want = svd_step(lambda **_: (as_unet_output(eps_c.double()),), lat.double(), 0, dtype=torch.float64, **kw)
        got = M.reference(d, t)["euler_out"].reshape(b, 4, fr, hh, ww)
        assert rel(got, want) <= 1e-6          # the oracle updates in fp32 whatever dtype it is given (2^-24 per operation)
        return
    eps_u = _rand(g, m, 8)
    scale = 2.5
    gs = torch.linspace(1.0, scale, fr)
    d.update(euler_eps_uncond=M.FAKE["euler_eps_uncond"], euler_guidance=M.FAKE["euler_guidance"], euler_ld_eps=8, euler_guidance_ld=guidance_ld)
    t.update(euler_eps_uncond=eps_u, euler_guidance=gs if guidance_ld == 0 else torch.cat([gs, torch.zeros(2), gs, torch.zeros(2)]))
    outs = iter([as_unet_output(eps_u[:, :4]), as_unet_output(eps_c)])        # the oracle runs the unconditional pass first
    want = svd_step(lambda **_: (next(outs),), lat.double(), 0, guidance_scale=scale, dtype=torch.float16, **kw)
    got = M.reference(d, t)["euler_out"].reshape(b, 4, fr, hh, ww)
    # the oracle mixes in fp16 (as documented) and then updates in fp32 and stores fp16: half an fp16 ulp of its rounding
    assert float(((got - want.double()).abs() / want.double().abs().clamp_min(1e-3)).max()) <= 2.0 ** -11 * 1.01


# ------------------------------------------------------------------------------------------------ legality
def _names(field, msg):
    return field.lower() in msg.lower()


def test_legality_table(submit):
    """Every descriptor of the table and one near-miss per rule: SP_EINVAL and a message that names the field; what the
    product passes: not refused."""
    failures = []
    for title, d, field in ILLEGAL_TABLE:
        assert M.legal(d) == (False, field), (title, M.legal(d))
        rc, msg = submit(d)
        if rc != -1 or not _names(field, msg):
            failures.append(f"{title}: rc={rc} {msg!r}")
    rng = random.Random(5)
    for name, field, _ok in M.RULES:
        d = M.draw(rng, None, (0, 0), legal_only=False, small=True, rule=name)
        ok, first = M.legal(d)
        assert not ok and name in M.broken_rules(d)
        rc, msg = submit(d)
        if rc != -1 or not _names(first, msg):
            failures.append(f"near-miss of {name} ({first}): rc={rc} {msg!r}")
    table = legal_table()
    assert len(table) >= 40
    seen = set()
    for d in table:
        assert M.legal(d) == (True, None), (M.legal(d), {k: v for k, v in d.items() if v})
        seen |= M.options_of(d)
        rc, msg = submit(d)
        if rc == -1:
            failures.append(f"legal descriptor refused: {msg!r} {({k: v for k, v in d.items() if v and k not in M.POINTERS})}")
    assert seen == set(M.OPTIONS), set(M.OPTIONS) - seen
    assert not failures, "\n" + "\n".join(failures)


def test_legality_differential(submit):
    """2,400 seeded draws, more than half of them with one rule broken: the library refuses exactly what legal() refuses."""
    rng = random.Random(20260)
    broken, n_legal, wrong = collections.Counter(), 0, []
    total = 2400
    for i in range(total):
        d = M.draw(rng, None, (rng.choice([0, 2, 3, 4]), 0), legal_only=False, small=True)
        ok, field = M.legal(d)
        assert ok == (d["_broken"] is None)
        n_legal += ok
        for name in M.broken_rules(d):
            broken[name] += 1
        rc, msg = submit(d)
        if (rc == -1) != (not ok):
            wrong.append(f"draw {i}: legal()={ok} ({d['_broken']}) but rc={rc} {msg!r}")
    assert n_legal >= 0.3 * total, n_legal
    assert all(broken[name] >= 10 for name in M.RULE_NAMES), sorted((broken[n], n) for n in M.RULE_NAMES)[:5]
    assert not wrong, f"{len(wrong)} disagreements:\n" + "\n".join(wrong[:20])


# ------------------------------------------------------------------------------------------------ the generator
def test_generator_coverage_and_rounding_floor():
    """Over the seeds the GPU fuzz uses: every option >= 10 times, every compatible pair >= 3 times, every mode with slack lda
    and with a batch >= 5 times; and the two error measures of an exact kernel with fp16 stores (reference().half() against
    reference()) stay <= 1e-3 for every draw, a third of the tolerance the fuzz applies."""
    opt, pair, trait = collections.Counter(), collections.Counter(), collections.Counter()
    worst = (0.0, 0.0)
    for route, d in M.fuzz_draws():
        assert M.legal(d) == (True, None)
        assert d["m"] * d["n"] * (M.TAPS[d["mode"]] * d["cin"] + d["cin2"]) <= 2e10
        o = sorted(M.options_of(d))
        opt.update(o)
        pair.update(frozenset((a, b)) for i, a in enumerate(o) for b in o[i + 1:])
        trait.update((d["mode"], t) for t in M.traits_of(d))
        _bufs, views = M.make_tensors(d)
        ref = M.reference(d, views)["d"]
        assert torch.isfinite(ref).all(), "a NaN slack column reached the reference"
        e = M.errors(ref.half(), ref)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
        assert max(e) <= 1e-3, (route, e, {k: v for k, v in d.items() if v})
    print(f"rounding floor over the fuzz draws: global {worst[0]:.2e}, worst block {worst[1]:.2e}")
    assert all(opt[o] >= 10 for o in M.OPTIONS), opt
    missing = [(a, b, pair[frozenset((a, b))]) for i, a in enumerate(M.OPTIONS) for b in M.OPTIONS[i + 1:]
               if M.compatible(a, b) and pair[frozenset((a, b))] < 3]
    assert not missing, missing
    assert all(trait[(mode, t)] >= 5 for mode in (M.LINEAR, M.CONV3X3, M.TEMPORAL3) for t in ("slack_lda", "batch")), trait
    assert trait[(M.LINEAR, "ragged_m")] >= 10


def test_block_measure_sees_what_the_global_one_hides():
    """5 % of the output's rms added to one 16 x 16 fragment of a large reference result: the global relative L2 error stays far
    below the tolerance (about 0.05 * sqrt(256 / elements)), the worst 64 x 64 block reads 0.05 * sqrt(256 / 4096) = 1.25e-2."""
    rng = random.Random(9)
    d = None
    while d is None or d["m"] < 4000 or d["n_store"] or d["geglu"] or d["euler_out"]:
        d = M.draw(rng, None, (3, 256))
    _bufs, views = M.make_tensors(d)
    ref = M.reference(d, views)["d"]
    rms = float(ref.pow(2).mean().sqrt())
    bad = ref.clone()
    bad[72:88, 100:116] += 0.05 * rms
    glob, block = M.errors(bad, ref)
    assert glob == pytest.approx(0.05 * math.sqrt(256 / ref.numel()), rel=1e-6) and glob <= M.TOL / 5
    assert block > M.TOL
    assert block == pytest.approx(0.05 * math.sqrt(256 / 4096), rel=1e-6)
    # a ragged border block is weighed by the elements it has: the same defect in the last rows reads no smaller
    if ref.shape[0] % 64 >= 16:
        bad = ref.clone()
        bad[-16:, :16] += 0.05 * rms
        assert M.errors(bad, ref)[1] == pytest.approx(0.05 * math.sqrt(256 / (ref.shape[0] % 64 * 64)), rel=1e-6)
    assert max(M.errors(ref.half(), ref)) <= 1e-3
