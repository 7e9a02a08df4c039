#!/usr/bin/env python3
"""The temporal VAE beyond 16,384 tokens per frame, timed on one GPU at the real widths, 14 frames in one chunk, random-init
weights:

  decode     the whole decode to uint8 frames at latents of 72x128 and 72x192 (short route: one [tokens][tokens] matrix, the
             register softmax) and of 108x192 and 72x256 (long route: query-row blocks, the streaming softmax), with
             torch.cuda.max_memory_allocated of each; host clock, one warm-up, median of three
  attention  the mid block's attention core of one frame at 20,736 tokens, split into its three calls, each over all row blocks
             (sp_gemm_f32out_f16, sp_softmax_rows_long_f32, sp_gemm_f16), device events, with FLOP and bytes counted from the shapes
  softmax    sp_softmax_rows_long_f32 against sp_softmax_rows_f32 at 9,216 and 16,384 columns, in place, 4,096 rows: the same
             bytes out, three reads of the row against one
  encode     the image encode at 864x1536

Nothing is asserted on these numbers.
usage: vae_long_timing.py [--launches 10] [--commit TEXT] [--out profiles/vae_long_timing.txt]"""
import argparse, math, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_long_timing.txt"))
args = ap.parse_args()
import torch
import vdpp_amd  # noqa
from vdpp_amd.hip import ops
from vdpp_amd.models.vae_hip import (ImageEncoderHIP, TemporalDecoderHIP, VAEDecoderConfig, attn_row_blocks,
                                     random_encoder_state_dict, random_state_dict)

F = 14


def events(fn, n):
    fn(); torch.cuda.synchronize()
    v = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); e1.synchronize()
        v.append(e0.elapsed_time(e1) / n)
    return statistics.median(v)                    # ms per call


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    cfg = VAEDecoderConfig.svd()
    dec = TemporalDecoderHIP(cfg, random_state_dict(cfg, seed=3, device=dev), dev)
    lines = []
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lines.append(f"device: {torch.cuda.get_device_name(0)}; commit: {commit or 'unknown'}; random-init full-width temporal VAE, {F} frames in one "
                 f"chunk, eager launches on one stream")
    lines.append("decode of the whole latent of one video to uint8 frames; host clock, one warm-up, median of three; peak = "
                 "torch.cuda.max_memory_allocated over the timed decodes (weights and latent included); scratch = the fp32 score matrix, counted:")
    for h, w in ((72, 128), (72, 192), (108, 192), (72, 256)):
        hw = h * w
        lat = torch.randn(1, 4, F, h, w, device=dev, dtype=torch.float16)
        v = []
        for i in range(4):
            if i == 1:
                torch.cuda.reset_peak_memory_stats(dev)
            torch.cuda.synchronize()
            t = time.perf_counter(); dec.decode_latents_uint8(lat, F, decode_chunk_size=F); torch.cuda.synchronize()
            v.append((time.perf_counter() - t) * 1e3)
        peak = torch.cuda.max_memory_allocated(dev)
        if hw > dec.attn_long_from:
            r, blocks = attn_row_blocks(hw, dec.attn_scratch_elems)
            route, scratch = f"long route, {len(blocks)} blocks of {r} rows", 4 * r * hw
        else:
            route, scratch = "short route", 4 * hw * hw
        lines.append(f"  latent {h}x{w:<4} ({hw:6d} tokens) -> {8 * h}x{8 * w} px  {statistics.median(v[1:]):8.1f} ms   peak {peak / 2**30:6.2f} GiB   "
                     f"scratch {scratch / 1e6:6.0f} MB   {route}")
        del lat
    torch.cuda.empty_cache()

    hw, c = 108 * 192, 512
    r, blocks = attn_row_blocks(hw)
    q = torch.randn(hw, c, device=dev, dtype=torch.float16)
    k = torch.randn(hw, c, device=dev, dtype=torch.float16)
    vt = torch.randn(c, hw, device=dev, dtype=torch.float16)
    o = torch.empty(hw, c, device=dev, dtype=torch.float16)
    s32 = torch.empty(r, hw, device=dev, dtype=torch.float32)
    p16 = s32.view(torch.float16)
    scale = 1.0 / math.sqrt(c)

    def qk():
        for r0, r1 in blocks:
            ops.gemm_f32out(q[r0:r1], k, s32, m=r1 - r0, n=hw, k=c)

    def sm():
        for r0, r1 in blocks:
            ops.softmax_rows_long_f32(s32, p16, rows=r1 - r0, cols=hw, scale=scale, ld=hw, ldo=2 * hw)

    def pv():
        for r0, r1 in blocks:
            ops.gemm(p16[:r1 - r0, :hw], vt, o[r0:r1], m=r1 - r0, n=c, cin=hw, lda=2 * hw)

    lines.append(f"attention core of ONE frame at {hw} tokens, width {c}, {len(blocks)} blocks of {r} query rows, each call over all blocks; device "
                 f"events around {args.launches} repeats, median of three; FLOP and bytes counted from the shapes (the softmax input is re-used, so "
                 f"its values are those of a softmax of probabilities: timing only):")
    t = events(qk, args.launches)
    lines.append(f"  sp_gemm_f32out_f16        S = Q K^T   {t:8.3f} ms   {2.0 * hw * hw * c / 1e9:7.1f} GFLOP -> {2.0 * hw * hw * c / t / 1e9:7.1f} TFLOP/s, "
                 f"{4.0 * hw * hw / 1e9:5.2f} GB written")
    qk()
    t = events(sm, args.launches)
    lines.append(f"  sp_softmax_rows_long_f32  in place    {t:8.3f} ms   {hw * hw * 14.0 / 1e9:5.2f} GB (three 4-byte reads, one 2-byte write) -> "
                 f"{hw * hw * 14.0 / t / 1e9:6.2f} TB/s")
    t = events(pv, args.launches)
    lines.append(f"  sp_gemm_f16               O = P V     {t:8.3f} ms   {2.0 * hw * hw * c / 1e9:7.1f} GFLOP -> {2.0 * hw * hw * c / t / 1e9:7.1f} TFLOP/s, "
                 f"{2.0 * hw * hw / 1e9:5.2f} GB read at a row pitch of {4 * hw} bytes")
    del q, k, vt, o, s32, p16

    lines.append(f"streaming softmax against the register kernel, 4,096 rows in place, the same bytes out; device events around {args.launches} "
                 f"launches, median of three; bytes counted (the register kernel reads the row once, the streaming kernel three times):")
    rows = 4096
    for cols in (9216, 16384):
        x = torch.randn(rows, cols, device=dev) * 8.0
        xh = x.view(torch.float16)
        t_reg = events(lambda: ops.softmax_rows_f32(x, xh, rows=rows, cols=cols, scale=scale, ld=cols, ldo=2 * cols), args.launches)
        t_long = events(lambda: ops.softmax_rows_long_f32(x, xh, rows=rows, cols=cols, scale=scale, ld=cols, ldo=2 * cols), args.launches)
        lines.append(f"  {cols:6d} columns   sp_softmax_rows_f32 {t_reg * 1e3:8.1f} us ({rows * cols * 6.0 / t_reg / 1e9:5.2f} TB/s of 6 bytes per logit)   "
                     f"sp_softmax_rows_long_f32 {t_long * 1e3:8.1f} us ({rows * cols * 14.0 / t_long / 1e9:5.2f} TB/s of 14 bytes per logit)   "
                     f"ratio {t_long / t_reg:.2f}")
        del x, xh
    del dec
    torch.cuda.empty_cache()

    enc = ImageEncoderHIP(cfg, random_encoder_state_dict(cfg, seed=4, device=dev), dev)
    img = torch.randn(1, 3, 864, 1536, device=dev).clamp(-1, 1).half()
    v = []
    for i in range(4):
        if i == 1:
            torch.cuda.reset_peak_memory_stats(dev)
        torch.cuda.synchronize()
        t = time.perf_counter(); enc.encode_image_latents(img, F); torch.cuda.synchronize()
        v.append((time.perf_counter() - t) * 1e3)
    lines.append(f"image encode at 864x1536 px (20,736 tokens in the mid block, long route), one image, host clock, one warm-up, median of three: "
                 f"{statistics.median(v[1:]):.1f} ms, peak {torch.cuda.max_memory_allocated(dev) / 2**30:.2f} GiB")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
