#!/usr/bin/env python3
"""Randomised cross-checks of the attention (UNet, CLIP), normalisation, LayerNorm-statistics, GEMV, row-softmax and GELU
kernels against fp32 / fp64 torch (CPU), with guard rows around every output (no write outside the rows the call owns).
``one_new`` draws the wide and pooled attention, the K/V pooling and the fp8 feed-forward kernels in a series of its own.
usage: fuzz_misc.py [cases] [seed]"""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
import vdpp_amd  # noqa
from vdpp_amd.hip import ops

DEV = "cuda"
G = 2


def h(t):
    return t.half().float()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def guarded(rows, cols):
    buf = torch.full((rows + 2 * G, cols), 9.0, dtype=torch.float16, device=DEV)
    return buf, buf[G:G + rows]


def check_guard(buf, rows, what):
    got = buf.float().cpu()
    assert torch.all(got[:G] == 9.0) and torch.all(got[G + rows:] == 9.0), "guard rows written: " + what
    assert torch.isfinite(got).all(), "non-finite output: " + what
    return got[G:G + rows]


def attn_spatial(rng, g, fp8):
    batch, heads = rng.choice([1, 2, 5]), rng.choice([1, 2, 5])
    seq = rng.choice([1, 5, 63, 64, 65, 127, 128, 129, 200, 577, 1000, 1153])
    c = heads * 64
    amp = rng.choice([0.5, 1.0, 2.0])
    qkv = h(torch.randn(batch * seq, 3 * c, generator=g) * amp)
    d = qkv.half().to(DEV)
    buf, o = guarded(batch * seq, c)
    kw = dict(ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, batch=batch, seq=seq, heads=heads)
    if fp8:
        ws = torch.empty(ops.attn_fp8_ws_bytes(batch, seq, heads), dtype=torch.uint8, device=DEV)
        ops.attn_spatial_fp8(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o, ws, **kw)
        x = qkv.clamp(-448, 448).to(torch.float8_e4m3fn).float()
        # ONE op-level bound for every row length and amplitude (DESIGN.md section 3, fp8 paragraph): 4e-2 relative L2
        # against fp32 attention of the e4m3-rounded inputs.  (2.2e-2 is what rounding P to e4m3 costs on long rows of
        # unit-variance inputs; peaked softmaxes and short rows average fewer rounded probabilities per output.)  The
        # 3e-2 of SURVEY 8c is asserted at the UNet boundary, where it is meaningful.
        tol = 4e-2
    else:
        ops.attn_spatial(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o, **kw)
        x, tol = qkv, 3e-3
    torch.cuda.synchronize()
    q, k, v = [t.reshape(batch, seq, heads, 64).transpose(1, 2) for t in x.split(c, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(batch * seq, c)
    what = f"attn_spatial{'_fp8' if fp8 else ''} batch={batch} seq={seq} heads={heads}"
    e = rel_l2(check_guard(buf, batch * seq, what), ref)
    assert e <= tol, f"rel_l2={e:.3e}: {what}"
    return e


def attn_long(rng, g):
    """Frozen-reference kernel: row lengths on both sides of its contract, amplitudes from flat to peaky, and (half of
    the cases) late keys that match a query far above its warm-up maximum, so that blocks take the second pass."""
    batch, heads = rng.choice([1, 2]), rng.choice([1, 2, 5])
    seq = rng.choice([4096, 4352, 4608, 5120, 4224, 4097, 2304])
    c = heads * 64
    amp = rng.choice([0.25, 1.0, 1.0, 2.0, 3.0])
    qkv = h(torch.randn(batch * seq, 3 * c, generator=g) * amp)
    qkv[:, 2 * c:] = h(qkv[:, 2 * c:] / amp)
    planted = rng.random() < 0.5
    if planted:
        x = qkv.view(batch, seq, 3 * heads, 64)
        for _ in range(rng.choice([1, 3, 20])):
            b, hd, qi, ki = rng.randrange(batch), rng.randrange(heads), rng.randrange(seq), rng.randrange(seq)
            x[b, ki, heads + hd] = h(x[b, qi, hd] * rng.choice([2.0, 3.0]) / max(amp * amp, 0.25))
    d = qkv.half().to(DEV)
    buf, o = guarded(batch * seq, c)
    ws = torch.full((ops.attn_long_ws_bytes(batch, seq, heads) // 4 + 1,), -1, dtype=torch.int32, device=DEV)
    ops.attn_spatial_long(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o, ws, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, batch=batch,
                          seq=seq, heads=heads)
    torch.cuda.synchronize()
    q, k, v = [t.reshape(batch, seq, heads, 64).transpose(1, 2) for t in qkv.split(c, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(batch * seq, c)
    what = f"attn_spatial_long batch={batch} seq={seq} heads={heads} amp={amp} planted={planted}"
    e = rel_l2(check_guard(buf, batch * seq, what), ref)
    assert e <= 3e-3, f"rel_l2={e:.3e}: {what}"
    assert int(ws[-1]) == -1, "flag words written past the workspace: " + what
    return e


def attn_temporal(rng, g):
    batch, heads, frames, hw = rng.choice([1, 2]), rng.choice([1, 3, 5]), rng.choice([1, 2, 14, 16, 17, 25, 32]), rng.choice([1, 3, 50, 257])
    c = heads * 64
    rows = batch * frames * hw
    qkv = h(torch.randn(rows, 3 * c, generator=g))
    d = qkv.half().to(DEV)
    buf, o = guarded(rows, c)
    ops.attn_temporal(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, batch=batch,
                      frames=frames, hw=hw, heads=heads)
    torch.cuda.synchronize()
    q, k, v = [t.reshape(batch, frames, hw, heads, 64).permute(0, 2, 3, 1, 4) for t in qkv.split(c, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v).permute(0, 3, 1, 2, 4).reshape(rows, c)
    what = f"attn_temporal batch={batch} frames={frames} hw={hw} heads={heads}"
    e = rel_l2(check_guard(buf, rows, what), ref)
    assert e <= 3e-3, f"rel_l2={e:.3e}: {what}"
    return e


def groupnorm(rng, g):
    inst = rng.choice([1, 2, 5, 14])
    rows = rng.choice([1, 7, 100, 144, 576, 577, 1000, 1632, 1633, 2304])
    c = rng.choice([64, 320, 640, 960, 1280, 1920, 2560])
    silu = rng.random() < 0.5
    eps = rng.choice([1e-5, 1e-6])
    x = h(torch.randn(inst, rows, c, generator=g) * rng.choice([0.3, 2.0]) + rng.choice([0.0, 0.7, -3.0]))
    gamma = torch.randn(c, generator=g); beta = torch.randn(c, generator=g)
    ref = F.group_norm(x.permute(0, 2, 1), 32, gamma, beta, eps=eps)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1).reshape(inst * rows, c)
    ws = torch.empty(ops.groupnorm_ws_bytes(inst, rows, c, 32), dtype=torch.uint8, device=DEV)
    buf, y = guarded(inst * rows, c)
    ops.groupnorm(x.half().to(DEV).reshape(inst * rows, c), gamma.to(DEV), beta.to(DEV), y, instances=inst, rows=rows, c=c,
                  groups=32, eps=eps, silu=silu, ws=ws)
    torch.cuda.synchronize()
    what = f"groupnorm inst={inst} rows={rows} c={c} silu={silu}"
    e = rel_l2(check_guard(buf, inst * rows, what), ref)
    assert e <= 3e-3, f"rel_l2={e:.3e}: {what}"
    return e


def layernorm(rng, g):
    rows = rng.choice([1, 3, 64, 257, 1000, 4099])
    c = rng.choice([64, 320, 640, 1280])
    x = h(torch.randn(rows, c, generator=g) * 2 + 0.5)
    gamma = torch.randn(c, generator=g); beta = torch.randn(c, generator=g)
    buf, y = guarded(rows, c)
    ops.layernorm(x.half().to(DEV), gamma.to(DEV), beta.to(DEV), y, rows=rows, c=c)
    torch.cuda.synchronize()
    what = f"layernorm rows={rows} c={c}"
    e = rel_l2(check_guard(buf, rows, what), F.layer_norm(x, (c,), gamma, beta))
    assert e <= 3e-3, f"rel_l2={e:.3e}: {what}"
    return e


def ln_stats(rng, g):
    rows = rng.choice([1, 3, 257, 4095, 4097, 8191, 8193, 9000, 20001])      # around the row-count thresholds of the
    c = rng.choice([64, 320, 640, 960, 1280])                                 # lane-group kernels (8192 / 4096 / 2048)
    x = h(torch.randn(rows, c, generator=g) * rng.choice([0.5, 3.0]) + 4.0 * torch.randn(rows, 1, generator=g))
    add = rng.random() < 0.4
    per = rng.choice([1, 50, 333])
    xd = x.half().to(DEV)
    st = torch.full((rows + 2, 2), -7.0, device=DEV)
    kw = {}
    if add:
        av = h(torch.randn((rows + per - 1) // per, c, generator=g))
        buf, sm = guarded(rows, c)
        kw = dict(addvec=av.half().to(DEV), addvec_rows=per, sum_out=sm)
        x = (x + av.repeat_interleave(per, 0)[:rows]).half().float()
    ops.ln_stats(xd, st[1:rows + 1], rows=rows, c=c, eps=1e-5, **kw)
    torch.cuda.synchronize()
    what = f"ln_stats rows={rows} c={c} add={add}"
    assert torch.all(st[0] == -7.0) and torch.all(st[rows + 1] == -7.0), "guard rows written: " + what
    if add:
        assert torch.equal(check_guard(buf, rows, what), x), "sum_out: " + what
    xd64 = x.double()
    got = st[1:rows + 1].cpu().double()
    assert float((got[:, 0] - xd64.mean(1)).abs().max()) < 1e-4, what
    e = rel_l2(got[:, 1], (xd64.var(1, unbiased=False) + 1e-5).rsqrt())
    assert e <= 1e-5, f"rstd rel_l2={e:.3e}: {what}"
    return e


def gemv(rng, g):
    batch, rows = rng.choice([1, 1, 3, 12]), rng.choice([1, 1, 2, 14])
    n, k = rng.choice([1, 7, 8, 9, 200, 203, 320, 1280, 5120]), rng.choice([64, 320, 1024, 1280])
    w = h(torch.randn(batch, n, k, generator=g) / k ** 0.5); b = torch.randn(batch, n, generator=g)
    shared = rng.random() < 0.5
    x = h(torch.randn(rows, k, generator=g)) if shared else h(torch.randn(batch, rows, k, generator=g))
    silu_in, silu_out = rng.random() < 0.3, rng.random() < 0.3
    xin = F.silu(x).half().float() if silu_in else x
    ref = (torch.einsum("rk,gnk->grn", xin, w) if shared else torch.einsum("grk,gnk->grn", xin, w)) + b[:, None, :]
    if silu_out: ref = F.silu(ref)
    flat = torch.full((batch * rows * n + 16,), 7.0, dtype=torch.float32, device=DEV)
    y = flat[8:8 + batch * rows * n].view(batch, rows, n)
    ops.gemv_batched(x.half().to(DEV), w.half().to(DEV), b.to(DEV), batch=batch, n=n, k=k, rows=rows,
                     x_stride=0 if shared else None, y32=y, silu_in=silu_in, silu_out=silu_out)
    torch.cuda.synchronize()
    what = f"gemv batch={batch} rows={rows} n={n} k={k} shared={shared} silu={silu_in}/{silu_out}"
    assert torch.all(flat[:8] == 7.0) and torch.all(flat[8 + batch * rows * n:] == 7.0), "guard written: " + what
    e = rel_l2(y.cpu(), ref)
    assert e <= 2e-3, f"rel_l2={e:.3e}: {what}"
    return e


def attn_small(rng, g):
    """CLIP-style attention: short sequences, any head width that is a multiple of 8 (K, V of a head must fit in LDS)."""
    import math
    batch, heads = rng.choice([1, 2, 3]), rng.choice([1, 2, 5, 16])
    hd = rng.choice([8, 40, 64, 80, 128])
    seq = rng.choice([1, 2, 63, 64, 65, 200, 257, 300])
    if seq * (hd + 1) * 4 > 140 * 1024:
        seq = 130
    c = heads * hd
    qkv = h(torch.randn(batch * seq, 3 * c, generator=g) * rng.choice([0.5, 1.0, 2.0]))
    d = qkv.half().to(DEV)
    buf, o = guarded(batch * seq, c)
    ops.attn_small(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], o, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, batch=batch, seq=seq,
                   heads=heads, head_dim=hd, scale=1.0 / math.sqrt(hd))
    torch.cuda.synchronize()
    q, k, v = [t.reshape(batch, seq, heads, hd).transpose(1, 2) for t in qkv.split(c, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(batch * seq, c)
    what = f"attn_small batch={batch} seq={seq} heads={heads} hd={hd}"
    e = rel_l2(check_guard(buf, batch * seq, what), ref)
    assert e <= 2e-3, f"rel_l2={e:.3e}: {what}"
    return e


def softmax_rows(rng, g):
    """The VAE mid block's in-place row softmax: any column count that is a multiple of 8 up to 16,384, row pitch >= it."""
    rows = rng.choice([1, 3, 64, 257])
    cols = rng.choice([8, 64, 264, 2048, 2056, 4104, 9216, 16384])
    ld = cols + rng.choice([0, 8, 64])
    x = h(torch.randn(rows, ld, generator=g) * rng.choice([0.5, 4.0, 30.0]))
    buf = torch.full((rows + 2 * G, ld), 9.0, dtype=torch.float16, device=DEV)
    buf[G:G + rows] = x.half().to(DEV)
    ops.softmax_rows(buf[G:G + rows], rows=rows, cols=cols, ld=ld)
    torch.cuda.synchronize()
    what = f"softmax_rows rows={rows} cols={cols} ld={ld}"
    got = check_guard(buf, rows, what)
    assert torch.equal(got[:, cols:], x[:, cols:]), "columns past cols touched: " + what
    ref = torch.softmax(x[:, :cols], dim=-1)
    assert float((got[:, :cols] - ref).abs().max()) <= 2e-3, what
    e = rel_l2(got[:, :cols], ref)
    assert e <= 2e-3, f"rel_l2={e:.3e}: {what}"
    return e


def gelu(rng, g):
    n = 8 * rng.choice([1, 37, 4096, 40001])
    x = h(torch.randn(n, generator=g) * rng.choice([0.5, 3.0, 8.0]))
    quick = rng.random() < 0.5
    buf = torch.full((n + 16,), 9.0, dtype=torch.float16, device=DEV)
    ops.gelu(x.half().to(DEV), buf[8:8 + n], quick=quick)
    torch.cuda.synchronize()
    got = buf.float().cpu()
    assert torch.all(got[:8] == 9.0) and torch.all(got[8 + n:] == 9.0), "gelu guard"
    ref = x * torch.sigmoid(1.702 * x) if quick else F.gelu(x)
    assert float((got[8:8 + n] - ref).abs().max()) <= 8e-3 and rel_l2(got[8:8 + n], ref) <= 1e-3, f"gelu n={n} quick={quick}"
    return 0.0


def one(rng, g):
    kind = rng.choice(["as", "as", "as8", "at", "gn", "gn", "ln", "lns", "lns", "gv", "asm", "asm", "sm", "gl", "al"])
    if kind == "al": return attn_long(rng, g)
    if kind == "asm": return attn_small(rng, g)
    if kind == "sm": return softmax_rows(rng, g)
    if kind == "gl": return gelu(rng, g)
    if kind == "lns": return ln_stats(rng, g)
    if kind == "gv": return gemv(rng, g)
    if kind == "as": return attn_spatial(rng, g, False)
    if kind == "as8": return attn_spatial(rng, g, True)
    if kind == "at": return attn_temporal(rng, g)
    if kind == "gn": return groupnorm(rng, g)
    return layernorm(rng, g)


# ------------------------------------------------------------------------------------------------ the newer kernels
# csrc/attention_wide.hip, csrc/attention_kv.hip, csrc/gemm_f8.hip.  Each kind is a pair: ``draw_<kind>(rng, g)`` builds
# the operands and the reference on the CPU (no kernel: tests/test_fuzz_draws_cpu.py runs the draws alone), ``<kind>(case)``
# runs the kernel.  Every operand with a row pitch is a column slice of a wider buffer whose slack is NaN (0x7F for e4m3
# bytes), every pitch of a call is different, every output sits between guard rows AND guard columns of a sentinel, and
# the call is made twice into fresh buffers: the two results are bit-identical.  They are drawn by ``one_new``, not by
# ``one``: the table of ``one`` decides which shapes a seed gives the older kinds.
E4M3 = torch.float8_e4m3fn
NEW_KINDS = ("kv_pool", "attn_spatial_kv", "attn_wide", "ln_quant_f8", "gemm_f8")


def slack(t, front, back):
    """CPU tensor [rows][cols] -> (wide buffer with NaN / 0x7F slack columns, column slice holding t)."""
    fill = 0x7F if t.dtype == torch.uint8 else float("nan")
    buf = torch.full((t.shape[0], front + t.shape[1] + back), fill, dtype=t.dtype)
    buf[:, front:front + t.shape[1]] = t
    return buf, slice(front, front + t.shape[1])


def on_device(t, front, back):
    """(device column slice of the slack buffer, its row pitch)."""
    buf, cols = slack(t, front, back)
    return buf.to(DEV)[:, cols], buf.shape[1]


def guarded2(rows, cols, front, back, dtype=torch.float16):
    """A sentinel-filled buffer with G guard rows above and below and ``front`` / ``back`` guard columns: (buffer, the
    [rows][cols] slice a call may write)."""
    buf = torch.full((rows + 2 * G, front + cols + back), 0x7F if dtype == torch.uint8 else 9.0, dtype=dtype, device=DEV)
    return buf, buf[G:G + rows, front:front + cols]


def check_guard2(buf, out, what):
    """The slice ``out`` of ``buf`` on the CPU after checking that nothing else was written and no NaN came out."""
    got = buf.cpu()
    rows, cols = out.shape
    front = out.storage_offset() % buf.shape[1]
    outside = torch.ones_like(got, dtype=torch.bool)
    outside[G:G + rows, front:front + cols] = False
    assert torch.all(got[outside] == (0x7F if got.dtype == torch.uint8 else 9.0)), "guard rows or columns written: " + what
    body = got[G:G + rows, front:front + cols]
    if got.dtype == torch.uint8:
        assert torch.all((body & 0x7F) != 0x7F), "a NaN code in the output: " + what
    else:
        assert torch.isfinite(body.float()).all(), "non-finite output: " + what
    return body


def twice(launch, what):
    """Runs ``launch() -> [(buffer, slice), ...]`` twice, checks guards, demands bit-identical results; the first run's."""
    runs = []
    for _ in range(2):
        outs = launch()
        torch.cuda.synchronize()
        runs.append([check_guard2(buf, out, what) for buf, out in outs])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b), \
            "two calls differ: " + what
    return runs[0]


def _edge_or_any(rng, edges, hi):
    return rng.choice(edges) if rng.random() < 0.5 else rng.randint(1, hi)


def draw_kv_pool(rng, g, f=None):
    """Multiples of 2^-6 with |x| <= 4: every partial sum of up to 16 of them is exact in fp32, so the order is free and the
    fp32 cell mean, rounded once, is the answer bit for bit.  Non-square grids: a swapped h / w shows."""
    f = rng.choice([2, 4]) if f is None else f
    while True:
        gh, gw = f * rng.randint(1, 16 // f), f * rng.randint(1, 24 // f)
        if gh != gw:
            break
    n_img, c = rng.randint(1, 3), rng.choice([64, 320, 640])
    k, v = [(torch.randint(-256, 257, (n_img * gh * gw, c), generator=g).float() / 64).half() for _ in range(2)]
    ref = [t.float().view(n_img, gh // f, f, gw // f, f, c).mean((2, 4)).reshape(-1, c).half() for t in (k, v)]
    return dict(kind="kv_pool", k=k, v=v, ref=ref, n_img=n_img, h=gh, w=gw, c=c, factor=f,
                what=f"kv_pool n_img={n_img} grid={gh}x{gw} c={c} factor={f}")


def kv_pool(case):
    c, what = case["c"], case["what"]
    rows = case["ref"][0].shape[0]
    (kd, ldk), (vd, ldv) = on_device(case["k"], 8, 16), on_device(case["v"], 24, 8)

    def launch():
        outs = [guarded2(rows, c, 8, 32), guarded2(rows, c, 16, 40)]
        ops.kv_pool(kd, vd, outs[0][1], outs[1][1], ldk=ldk, ldv=ldv, ldkp=outs[0][0].shape[1], ldvp=outs[1][0].shape[1],
                    n_img=case["n_img"], h=case["h"], w=case["w"], c=c, factor=case["factor"])
        assert len({ldk, ldv, outs[0][0].shape[1], outs[1][0].shape[1]}) == 4
        return outs
    for got, ref, name in zip(twice(launch, what), case["ref"], "kv"):
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), f"{name}p is not the fp32 cell mean: {what}"
    return 0.0


def _softmax_fp64(q, k, v, scale):
    return torch.softmax(q.double() @ k.double().transpose(-1, -2) * scale, dim=-1) @ v.double()


def draw_attn_spatial_kv(rng, g):
    batch, heads = rng.randint(1, 3), rng.randint(1, 5)
    seq_q = _edge_or_any(rng, [1, 33, 255, 256, 257, 511, 512, 513, 600], 600)
    seq_kv = _edge_or_any(rng, [1, 63, 64, 65, 127, 128, 129, 192, 300], 300)
    c, amp = heads * 64, rng.choice([0.5, 1.0, 2.0])
    q = (torch.randn(batch * seq_q, c, generator=g) * amp).half()
    k, v = (torch.randn(batch * seq_kv, c, generator=g) * amp).half(), torch.randn(batch * seq_kv, c, generator=g).half()
    split = lambda t, n: t.view(batch, n, heads, 64).transpose(1, 2)
    ref = _softmax_fp64(split(q, seq_q), split(k, seq_kv), split(v, seq_kv), 0.125).transpose(1, 2).reshape(batch * seq_q, c)
    return dict(kind="attn_spatial_kv", q=q, k=k, v=v, ref=ref, batch=batch, heads=heads, seq_q=seq_q, seq_kv=seq_kv,
                what=f"attn_spatial_kv batch={batch} seq_q={seq_q} seq_kv={seq_kv} heads={heads} amp={amp}")


def attn_spatial_kv(case):
    what, c = case["what"], case["heads"] * 64
    (qd, ldq), (kd, ldk), (vd, ldv) = on_device(case["q"], 8, 8), on_device(case["k"], 16, 24), on_device(case["v"], 24, 48)

    def launch():
        buf, o = guarded2(case["q"].shape[0], c, 8, 56)
        assert len({ldq, ldk, ldv, buf.shape[1]}) == 4
        ops.attn_spatial_kv(qd, kd, vd, o, ldq=ldq, ldk=ldk, ldv=ldv, ldo=buf.shape[1], batch=case["batch"], seq_q=case["seq_q"],
                            seq_kv=case["seq_kv"], heads=case["heads"])
        return [(buf, o)]
    e = rel_l2(twice(launch, what)[0].float(), case["ref"])
    assert e <= 3e-3, f"rel_l2={e:.3e}: {what}"
    return e


def draw_attn_wide(rng, g, d=None):
    d, batch = rng.choice([128, 256, 512]) if d is None else d, rng.randint(1, 2)
    seq = _edge_or_any(rng, [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300], 300)
    q, k, v = [torch.randn(batch * seq, d, generator=g).half() for _ in range(3)]
    bias = torch.randn(d, generator=g) if rng.random() < 0.5 else None
    ref = _softmax_fp64(*[t.view(batch, seq, d) for t in (q, k, v)], d ** -0.5).reshape(batch * seq, d)
    if bias is not None:
        ref = ref + bias.double()
    return dict(kind="attn_wide", q=q, k=k, v=v, bias=bias, ref=ref, batch=batch, seq=seq, d=d,
                what=f"attn_wide d={d} batch={batch} seq={seq} bias={bias is not None}")


def attn_wide(case):
    what, d = case["what"], case["d"]
    (qd, ldq), (kd, ldk), (vd, ldv) = on_device(case["q"], 8, 8), on_device(case["k"], 16, 24), on_device(case["v"], 24, 48)
    bias = None if case["bias"] is None else case["bias"].to(DEV)

    def launch():
        buf, o = guarded2(case["q"].shape[0], d, 8, 56)
        assert len({ldq, ldk, ldv, buf.shape[1]}) == 4
        ops.attn_wide(qd, kd, vd, o, ldq=ldq, ldk=ldk, ldv=ldv, ldo=buf.shape[1], batch=case["batch"], seq=case["seq"], head_dim=d,
                      scale=d ** -0.5, bias=bias)
        return [(buf, o)]
    e = rel_l2(twice(launch, what)[0].float(), case["ref"])
    assert e <= 3e-3, f"rel_l2={e:.3e}: {what}"
    return e


def draw_ln_quant_f8(rng, g):
    """The statistics are computed here (fp64, stored as the fp32 pair the kernel reads), so the criterion is a property
    of sp_ln_quant_f8 alone: y in fp64 from those very numbers."""
    c, rows = 64 * rng.randint(1, 20), _edge_or_any(rng, [1, 2, 15, 16, 17, 63, 64, 65, 300], 300)
    x = (torch.randn(rows, c, generator=g) * rng.choice([0.3, 1.0, 4.0]) + rng.choice([0.0, 0.7, -3.0])).half()
    if rng.random() < 0.5:
        x[0, rng.randrange(c)] = 1000.0                         # one spike: every other byte of the row is tiny
    if rows > 1 and rng.random() < 0.5:
        x[1] = 0.5                                              # a constant row: amax = 0, zeros with sa = 1
    xd = x.double()
    st = torch.stack([xd.mean(1), (xd.var(1, unbiased=False) + 1e-5).rsqrt()], 1).float()
    y = (xd - st[:, :1].double()) * st[:, 1:].double()
    return dict(kind="ln_quant_f8", x=x, st=st, y=y, rows=rows, c=c, constant_row=bool(rows > 1 and (x[1] == 0.5).all()),
                what=f"ln_quant_f8 rows={rows} c={c}")


def ln_quant_f8(case):
    what, rows, c, y = case["what"], case["rows"], case["c"], case["y"]
    xd, ldx = on_device(case["x"], 8, 24)
    st = case["st"].to(DEV)

    runs = []
    for _ in range(2):
        qbuf, q = guarded2(rows, c, 16, 48, dtype=torch.uint8)
        sbuf = torch.full((rows + 2 * G,), 9.0, device=DEV)                # (fp32: guard words in front and behind)
        assert ldx != qbuf.shape[1] and ldx > c and qbuf.shape[1] > c
        ops.ln_quant_f8(xd, st, q, sbuf[G:G + rows], rows=rows, c=c, ldx=ldx, ldq=qbuf.shape[1])
        torch.cuda.synchronize()
        sa = sbuf.cpu()
        assert torch.all(sa[:G] == 9.0) and torch.all(sa[G + rows:] == 9.0), "guard words of sa written: " + what
        assert torch.isfinite(sa).all(), "non-finite sa: " + what
        runs.append((check_guard2(qbuf, q, what), sa[G:G + rows]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two calls differ: " + what
    q, sa = runs[0]
    amax = y.abs().amax(1)
    want_sa = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).float()
    spacing = torch.nextafter(want_sa, torch.full_like(want_sa, float("inf"))) - want_sa
    ulps = (sa.double() - want_sa.double()).abs() / spacing.double()
    assert float(ulps.max()) <= 2.0, f"sa is {float(ulps.max())} ulp off: {what}"
    if case["constant_row"]:
        assert float(sa[1]) == 1.0 and bool((q[1] == 0).all()), "constant row: " + what
    err = (q.view(E4M3).double() * sa.double()[:, None] - y).abs()
    allowed = 2.0 ** -4 * y.abs() + sa.double()[:, None] * 2.0 ** -10
    assert bool((err <= allowed).all()), "more than half an e4m3 step: " + what
    return float((err / allowed).max())


GEMM_F8_K = (64, 128, 192, 320, 640, 1280)


def gemm_f8_tiles(case):
    return (case["m"] + 255) // 256, (case["n"] + 255) // 256


def draw_gemm_f8(rng, g, big=None, k=None, mode=None):
    """``big``: at least 3 x 3 workgroup tiles (256 rows x 256 weight rows each); ``k``: that depth.  Plain and residual
    draws carry the integer operands of tests/test_gemm_f8_gpu.py (A, W in {-1, 0, 1}, scales in {1/2, 1}, integer bias and
    residual): every partial sum is a multiple of 1/4 far below 2^24, so the fp64 reference is its own fp16 rounding and
    the kernel must EQUAL it.  GEGLU draws are Gaussian, packed by models/weights.py."""
    from vdpp_amd.models import weights as W
    mode = rng.choice(["plain", "res", "geglu"]) if mode is None else mode
    big = rng.random() < 0.4 if big is None else big
    tm, tn = (rng.randint(3, 5), rng.randint(3, 5)) if big else (rng.randint(1, 5), rng.randint(1, 5))
    m = rng.randint(256 * (tm - 1) + 1, min(256 * tm, 1100))
    n = 128 * rng.randint(2 * tn - 1, 2 * tn)
    k = rng.choice(GEMM_F8_K) if k is None else k
    case = dict(kind="gemm_f8", mode=mode, m=m, n=n, k=k, res=None, what=f"gemm_f8 {mode} m={m} n={n} k={k}")
    dec = lambda b: b.view(E4M3).double()
    if mode == "geglu":
        a, w, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g)
        sa = a.abs().amax(1) / 448.0
        a8 = (a / sa[:, None]).to(E4M3).view(torch.uint8)
        w8, sw = W.pack_linear_f8(w, geglu=False)
        w8i, swi = W.pack_linear_f8(w, geglu=True)
        _, bi = W.interleave_geglu(w, b)
        yy = sa.double()[:, None] * sw.double()[None, :] * (dec(a8) @ dec(w8).t()) + b.double()
        case.update(a8=a8, sa=sa, w8=w8i, sw=swi, bias=bi, ref=yy[:, :n // 2] * F.gelu(yy[:, n // 2:]))
        return case
    code = torch.tensor([0xB8, 0x00, 0x38], dtype=torch.uint8)           # -1, 0, 1
    a8, w8 = code[torch.randint(0, 3, (m, k), generator=g)], code[torch.randint(0, 3, (n, k), generator=g)]
    sa, sw = 0.5 * torch.randint(1, 3, (m,), generator=g).float(), 0.5 * torch.randint(1, 3, (n,), generator=g).float()
    bias = torch.randint(-8, 9, (n,), generator=g).float()
    # (operands in {-1, 0, 1}, at most 1,280 terms: the fp32 product is exact)
    ref = sa.double()[:, None] * sw.double()[None, :] * (a8.view(E4M3).float() @ w8.view(E4M3).float().t()).double() + bias.double()
    if mode == "res":
        case["res"] = torch.randint(-4, 5, (m, n), generator=g).half()
        ref = ref + 2.0 * case["res"].double()
    case.update(a8=a8, sa=sa, w8=w8, sw=sw, bias=bias, ref=ref)
    return case


def gemm_f8(case):
    what, m, n, k, geglu = case["what"], case["m"], case["n"], case["k"], case["mode"] == "geglu"
    nout = n // 2 if geglu else n
    a8, lda = on_device(case["a8"], 16, 48)
    r1, ldr1 = on_device(case["res"], 8, 16) if case["res"] is not None else (None, None)
    sa, w8, sw, bias = [case[key].to(DEV) for key in ("sa", "w8", "sw", "bias")]

    def launch():
        buf, d = guarded2(m, nout, 8, 40)
        assert lda > k and buf.shape[1] > nout and (r1 is None or ldr1 > n and ldr1 != buf.shape[1])
        ops.gemm_f8(a8, sa, w8, sw, bias, d, m=m, n=n, k=k, geglu=geglu, res1=r1, r1scale=2.0, lda=lda, ldd=buf.shape[1], ldr1=ldr1)
        return [(buf, d)]
    got, ref = twice(launch, what)[0], case["ref"]
    if not geglu:
        assert torch.equal(ref.half().double(), ref), "the reference is not exactly representable in fp16: " + what
        assert torch.equal(got.view(torch.int16), ref.half().view(torch.int16)), "not equal to the integer reference: " + what
        return 0.0
    got = got.double()
    l2, mx = float((got - ref).norm() / ref.norm()), float((got - ref).abs().max() / ref.abs().max())
    assert l2 <= 2e-3 and mx <= 1e-2, f"rel_l2={l2:.3e} max_rel={mx:.3e}: {what}"
    return l2


NEW_SEED, NEW_DRAWS = 424, 60         # the series of tests/test_fuzz_gpu.py::test_new_kernel_fuzz (and of its CPU dry run)


def draw_new(rng, g, i):
    """Draw ``i`` of a series: the five kinds in turn.  Of the sp_gemm_f8 draws every second has at least 3 x 3 tiles and
    every fourth K = 640, the others walk the depths and all of them the three epilogues; the sp_attn_wide_f16 draws take
    the three head widths in turn and the sp_kv_pool_f16 draws the two factors (a seed cannot miss the coverage the test
    asserts).  Everything else is the seed's."""
    kind, j = NEW_KINDS[i % len(NEW_KINDS)], i // len(NEW_KINDS)
    if kind == "gemm_f8":
        return draw_gemm_f8(rng, g, big=True if j % 2 == 0 else None, k=640 if j % 4 == 1 else GEMM_F8_K[j % len(GEMM_F8_K)],
                            mode=("plain", "res", "geglu")[j % 3])
    if kind == "kv_pool":
        return draw_kv_pool(rng, g, f=(2, 4)[j % 2])
    if kind == "attn_wide":
        return draw_attn_wide(rng, g, d=(128, 256, 512)[j % 3])
    return globals()["draw_" + kind](rng, g)


def one_new(rng, g, i):
    """-> (case, its error measure: rel-L2 for the attention and GEGLU kinds, the worst share of the allowed half step for
    ln_quant_f8, 0 for the kinds held exact)."""
    case = draw_new(rng, g, i)
    return case, globals()[case["kind"]](case)


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng, g = random.Random(seed), torch.Generator().manual_seed(seed)
    for i in range(cases):
        one(rng, g)
        if (i + 1) % 25 == 0:
            print(f"{i + 1} cases ok", flush=True)
    print(f"fuzz_misc: {cases} cases passed (seed {seed})")


if __name__ == "__main__":
    main()
