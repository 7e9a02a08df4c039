// Lossless WebP (VP8L) streams of uint8 frames that are already in device memory: the still and animated .webp output of
// save_frames.  The library makes, per frame, the complete VP8L bitstream from its signature byte on; the RIFF container has
// no checksum, so the host only wraps bytes (models/image_io.py webp_file / write_webp).  include/svdpipe.h fixes the rules,
// tests/webp_model.py restates them.  The frame is lossless, so every prediction comes from original pixels and no stage
// waits for a reconstruction.
//
//   webp_cost_kernel      : a workgroup per row: the two sums that decide the subtract-green transform, added per frame.
//   webp_transform_kernel : a workgroup per block row, a thread per column of a group of max(256, block) columns: the 14 sums
//                           of min(b, 256 - b) per block by LDS atomics, the choice, then the residual pixels.  A thread
//                           walks its column downwards and keeps the three pixels above it from the row before.
//   webp_strip_kernel     : a workgroup per (frame, strip of 2^group_bits rows) with five prefix codes of its own.  The strip
//                           passes through LDS twice in chunks of 2048 pixels, 8 consecutive pixels per thread; the token at a
//                           position follows from the start of its run of equal pixels exactly as in png_deflate_kernel, with
//                           copies of up to 4096 pixels.  First pass: the histograms of green (with the length symbols), red
//                           and blue by LDS atomics.  Then each code: the simple form, or png.hip's builder (codec_common.h
//                           holds it for both), the run-length form of its lengths and the 19-symbol code.  Second pass: bits per token, a prefix sum, and every token ORed into an LDS
//                           image of the chunk's words.  The code header and the pixel bits go to separate staging segments.
//   webp_head_kernel      : two workgroups per frame with the same coder: the header, the transforms and the mode image; the
//                           main image's first bits and the entropy image that gives block row g the code group g.
//   webp_scan_kernel      : per frame the exclusive sum of the 2 + 2G segments' bit counts, out_len.
//   webp_place_kernel     : one workgroup per segment writes the bytes whose first bit lies in the segment (png_place_kernel's
//                           rule; a segment here may be shorter than a byte, so a byte's missing bits are gathered from as many
//                           following segments as it takes).
// No workgroup waits for another inside a kernel; the launches are joined by stream order.  Nothing here is tuned beyond its
// layout; profiles/webp_timing.txt has what it costs.
#include "codec_common.h"

namespace {

constexpr int MAX_PIXELS = 1 << 24, MAX_SIDE = 16384;
constexpr int NSYM = 280, NCL = 19;                          // green's alphabet: 256 literals and 24 length prefixes
constexpr int MAX_COPY = 4096;
constexpr int CHUNK = 2048, PER = 8;
constexpr int normal_bits(int alphabet) { return 1 + 4 + 19 * 3 + 1 + alphabet * 14; }
constexpr int SIMPLE_1BIT = 4, SIMPLE_8BIT = 11;
constexpr int GROUP_HEADER_MAX = normal_bits(280) + 2 * normal_bits(256) + 2 * SIMPLE_1BIT;
constexpr int SUB_HEADER_MAX = normal_bits(280) + normal_bits(256) + SIMPLE_1BIT + SIMPLE_8BIT + SIMPLE_1BIT;
constexpr int MAIN_PIXEL_BITS_MAX = 45, SUB_PIXEL_BITS_MAX = 30;
constexpr int PREAMBLE_BITS_MAX = 64;
// the larger of: a group's code header; a sub-image's preamble, code header and one chunk; one chunk of the main image
constexpr int OWORDS = (PREAMBLE_BITS_MAX + GROUP_HEADER_MAX + CHUNK * MAIN_PIXEL_BITS_MAX) / 32 + 8;

__constant__ u8 CL_ORDER[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

bool webp_dims_ok(int h, int w) { return h > 0 && w > 0 && h <= MAX_SIDE && w <= MAX_SIDE && (int64_t)h * w <= MAX_PIXELS; }
bool webp_bits_ok(int pred_bits, int group_bits) {
  return pred_bits >= 2 && pred_bits <= 9 && (group_bits == 0 || (group_bits >= 2 && group_bits <= 9));
}

// ---------------------------------------------------------------------------------------------- subtract green?
// grid: one workgroup of 256 per row of every frame; sums[2 f] with green taken out, sums[2 f + 1] plain
__global__ __launch_bounds__(256) void webp_cost_kernel(const u8 *__restrict__ frames, int h, int w, u64 *__restrict__ sums) {
  __shared__ u32 red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t row = blockIdx.x;
  const u8 *cur = frames + row * 3 * w;
  u32 with = 0, plain = 0;
  for (int x = 1 + tid; x < w; x += 256) {
    const int r0 = cur[3 * x - 3], g0 = cur[3 * x - 2], b0 = cur[3 * x - 1], r1 = cur[3 * x], g1 = cur[3 * x + 1], b1 = cur[3 * x + 2];
    plain += byte_cost(r1 - r0) + byte_cost(b1 - b0);
    with += byte_cost((r1 - g1) - (r0 - g0)) + byte_cost((b1 - g1) - (b0 - g0));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    with += __shfl_xor(with, o, 64);
    plain += __shfl_xor(plain, o, 64);
  }
  if (lane == 0) { red[wv][0] = with; red[wv][1] = plain; }
  __syncthreads();
  if (tid < 2) atomicAdd(&sums[2 * (row / h) + tid], (u64)red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]);
}

// ---------------------------------------------------------------------------------------------- predictor transform
// a pixel as R << 16 | G << 8 | B, green taken out of red and blue if sg
__device__ __forceinline__ u32 load_px(const u8 *__restrict__ frame, int64_t p, bool sg) {
  int r = frame[3 * p], g = frame[3 * p + 1], b = frame[3 * p + 2];
  if (sg) { r = (r - g) & 255; b = (b - g) & 255; }
  return (u32)(r << 16 | g << 8 | b);
}
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ bool select_left(u32 L, u32 T, u32 TL) {
  int to_left = 0, to_top = 0;                               // sum |T - TL| is the distance of L + T - TL from L
#pragma unroll
  for (int c = 0; c < 24; c += 8) {
    const int l = (L >> c) & 255, t = (T >> c) & 255, tl = (TL >> c) & 255;
    to_left += abs(t - tl);
    to_top += abs(l - tl);
  }
  return to_left < to_top;
}
// one channel of the format's predictor `mode`; (a - tl) / 2 truncates toward zero
__device__ __forceinline__ int predict_channel(int mode, int l, int t, int tl, int tr, bool pick_left) {
  switch (mode) {
    case 0: return 0;
    case 1: return l;
    case 2: return t;
    case 3: return tr;
    case 4: return tl;
    case 5: return (((l + tr) >> 1) + t) >> 1;
    case 6: return (l + tl) >> 1;
    case 7: return (l + t) >> 1;
    case 8: return (tl + t) >> 1;
    case 9: return (t + tr) >> 1;
    case 10: return (((l + tl) >> 1) + ((t + tr) >> 1)) >> 1;
    case 11: return pick_left ? l : t;
    case 12: return clamp255(l + t - tl);
    default: { const int a = (l + t) >> 1; return clamp255(a + (a - tl) / 2); }
  }
}

// grid: one workgroup of 256 per block row of every frame
__global__ __launch_bounds__(256) void webp_transform_kernel(const u8 *__restrict__ frames, int h, int w, int pred_bits, int bh, int bw,
                                                             const u64 *__restrict__ sums, int *__restrict__ flags,
                                                             u8 *__restrict__ modes, u32 *__restrict__ residual) {
  __shared__ u32 block_sum[64][14];
  __shared__ u8 block_mode[64];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x / bh;
  const int by = (int)(blockIdx.x % bh);
  const int bs = 1 << pred_bits, y0 = by * bs, y1 = min(h, y0 + bs);
  const int group = max(256, bs), blocks = group >> pred_bits;           // columns and blocks of one pass; blocks <= 64
  const bool sg = sums[2 * f] < sums[2 * f + 1];                         // ties take the plain form
  if (by == 0 && tid == 0) flags[f] = sg ? 1 : 0;
  const int64_t total = (int64_t)h * w;
  const u8 *frame = frames + f * total * 3;
  u32 *res = residual + f * total;
  u8 *mode_row = modes + (f * bh + by) * bw;

  for (int x0 = 0; x0 < w; x0 += group) {
    for (int i = tid; i < 64 * 14; i += 256) (&block_sum[0][0])[i] = 0;
    __syncthreads();
    // ---- the 14 sums of every block; the first row and the first column do not depend on the mode and stay out
    for (int x = x0 + tid; x < min(w, x0 + group); x += 256) {
      if (x == 0) continue;
      u32 s[14];
#pragma unroll
      for (int m = 0; m < 14; ++m) s[m] = 0;
      const int ya = max(y0, 1);
      int64_t p = (int64_t)(ya - 1) * w + x;
      u32 TL = 0, T = 0, TR = 0;
      if (ya < y1) { TL = load_px(frame, p - 1, sg); T = load_px(frame, p, sg); TR = load_px(frame, p + 1, sg); }
      for (int y = ya; y < y1; ++y) {
        p += w;
        const u32 L = load_px(frame, p - 1, sg), X = load_px(frame, p, sg), N = p + 1 < total ? load_px(frame, p + 1, sg) : 0u;
        const bool pick_left = select_left(L, T, TL);
#pragma unroll
        for (int c = 0; c < 24; c += 8) {
          const int v = (X >> c) & 255, l = (L >> c) & 255, t = (T >> c) & 255, tl = (TL >> c) & 255, tr = (TR >> c) & 255;
#pragma unroll
          for (int m = 0; m < 14; ++m) s[m] += byte_cost(v - predict_channel(m, l, t, tl, tr, pick_left));
        }
        TL = L; T = X; TR = N;
      }
      const int b = (x - x0) >> pred_bits;
#pragma unroll
      for (int m = 0; m < 14; ++m)
        if (s[m]) atomicAdd(&block_sum[b][m], s[m]);
    }
    __syncthreads();
    if (tid < blocks && x0 + (tid << pred_bits) < w) {
      int best = 0;
      u32 best_sum = block_sum[tid][0];
      for (int m = 1; m < 14; ++m)
        if (block_sum[tid][m] < best_sum) { best_sum = block_sum[tid][m]; best = m; }   // (strictly less: the lower mode among equals)
      block_mode[tid] = (u8)best;
      mode_row[(x0 >> pred_bits) + tid] = (u8)best;
    }
    __syncthreads();
    // ---- the residuals
    for (int x = x0 + tid; x < min(w, x0 + group); x += 256) {
      const int mode = block_mode[(x - x0) >> pred_bits];
      int64_t p = (int64_t)(y0 - 1) * w + x;
      u32 TL = 0, T = 0, TR = 0;
      if (y0 > 0) { TL = x > 0 ? load_px(frame, p - 1, sg) : 0u; T = load_px(frame, p, sg); TR = load_px(frame, p + 1, sg); }
      for (int y = y0; y < y1; ++y) {
        p += w;
        const u32 L = p > 0 ? load_px(frame, p - 1, sg) : 0u, X = load_px(frame, p, sg), N = p + 1 < total ? load_px(frame, p + 1, sg) : 0u;
        u32 pred;
        if (y == 0) pred = x == 0 ? 0u : L;                   // the top-left pixel predicts 0xff000000, the top row L
        else if (x == 0) pred = T;                            // the left column T
        else {
          const bool pick_left = mode == 11 && select_left(L, T, TL);
          pred = 0;
#pragma unroll
          for (int c = 0; c < 24; c += 8)
            pred |= (u32)predict_channel(mode, (L >> c) & 255, (T >> c) & 255, (TL >> c) & 255, (TR >> c) & 255, pick_left) << c;
        }
        u32 out = 0;
#pragma unroll
        for (int c = 0; c < 24; c += 8) out |= ((((X >> c) & 255u) - ((pred >> c) & 255u)) & 255u) << c;
        res[p] = out;                                         // bytes B, G, R and alpha's residual, which is always 0
        TL = L; T = X; TR = N;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- the coder of one image
// (the code construction, HuffBuilder and what works on it, is in codec_common.h: the builder deflate has)
struct Strip {
  u32 buf[CHUNK + 4];                   // [0]: the pixel before the chunk; [1 ..): the chunk and two pixels behind it
  u32 obuf[OWORDS];
  HuffBuilder<NSYM> B;
  u32 hist_g[NSYM], hist_r[256], hist_b[256];
  u8 len_g[NSYM], len_r[256], len_b[256];
  u16 code_g[NSYM], code_r[256], code_b[256];
  u8 cl_len[NCL];
  u16 cl_code[NCL];
  u16 seq[NSYM + 2];                    // the run-length form: symbol | extra value << 5
  int nseq, at, used, only;
  int wave_val[4];
  int run_carry;
};

// where an image's pixels come from: the residuals (alpha is coded as 0), the mode image, the entropy image
struct MainSrc {
  const u32 *px;
  __device__ __forceinline__ u32 operator()(int q) const { return px[q] & 0x00ffffffu; }
};
struct ModeSrc {
  const u8 *mode;
  __device__ __forceinline__ u32 operator()(int q) const { return 0xff000000u | ((u32)mode[q] << 8); }
};
struct GroupSrc {
  int across;
  __device__ __forceinline__ u32 operator()(int q) const {
    const u32 g = (u32)(q / across);
    return 0xff000000u | ((g >> 8) << 16) | ((g & 255u) << 8);
  }
};

// one thread: behind the S.at bits in S.obuf
__device__ __forceinline__ void put_bits(Strip &S, u32 value, int width) { ::put_bits(S.obuf, S.at, value, width); }

// the prefix symbol of a copy's length: symbol | extra bits << 8 | extra value << 16
__device__ __forceinline__ u32 length_prefix(int length) {
  const u32 d = (u32)length - 1;
  if (d < 4) return d;
  const int hb = 31 - __clz(d), eb = hb - 1;
  return (u32)(2 * hb + ((d >> eb) & 1u)) | ((u32)eb << 8) | ((d & ((1u << eb) - 1)) << 16);
}

template <class Src>
__device__ __forceinline__ void load_chunk(Strip &S, const Src &src, int c0, int total) {
  __syncthreads();
  for (int i = threadIdx.x; i < CHUNK + 3; i += 256) {
    const int q = c0 - 1 + i;
    S.buf[i] = (q >= 0 && q < total) ? src(q) : 0u;
  }
  __syncthreads();
}

// tok[i] for the thread's positions c0 + 8 tid + i: -1 none, 0 a literal (val[i]), >= 3 a copy of that length
template <class Src>
__device__ __forceinline__ void chunk_tokens(Strip &S, const Src &src, int c0, int total, int (&tok)[PER], u32 (&val)[PER]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p0 = c0 + tid * PER;
  u32 px[PER + 3];                                           // px[k]: the pixel at p0 - 1 + k
#pragma unroll
  for (int k = 0; k < PER + 3; ++k) px[k] = S.buf[tid * PER + k];
  u32 flags = 0;
  int last = -1;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int p = p0 + i;
    val[i] = px[i + 1];
    if (p < total && (p == 0 || px[i + 1] != px[i])) { flags |= 1u << i; last = p; }
  }
  // where the run that reaches this thread's first position started
  int incl = last;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl = max(incl, up);
  }
  int start = __shfl_up(incl, 1, 64);
  if (lane == 0) start = -1;
  if (lane == 63) S.wave_val[wv] = incl;
  __syncthreads();
  start = max(start, S.run_carry);
  for (int i = 0; i < wv; ++i) start = max(start, S.wave_val[i]);
  __syncthreads();
  if (tid == 255) S.run_carry = max(start, last);
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int p = p0 + i;
    tok[i] = -1;
    if (p >= total) continue;
    const u32 v = px[i + 1];
    if (flags & (1u << i)) { start = p; tok[i] = 0; continue; }
    const int jm = (p - start - 1) % MAX_COPY;
    if (jm == 0) {
      const bool three = p + 2 < total && px[i + 2] == v && px[i + 3] == v;
      if (!three) tok[i] = 0;
      else {
        const int lim = min(MAX_COPY, total - p);
        int r = 3;
        while (r < lim && src(p + r) == v) ++r;
        tok[i] = r;
      }
    } else if (jm == 1) {
      if (p + 1 >= total || px[i + 2] != v) tok[i] = 0;
    }
  }
}

// one thread: the simple form of a code with the one symbol `sym`
__device__ __forceinline__ void put_simple_code(Strip &S, int sym) {
  put_bits(S, 1, 1);
  put_bits(S, 0, 1);
  if (sym < 2) { put_bits(S, 0, 1); put_bits(S, (u32)sym, 1); }
  else { put_bits(S, 1, 1); put_bits(S, (u32)sym, 8); }
}

// Every thread: one prefix code from hist[0 .. nsym) appended to the bits in S.obuf; its lengths and codes for the tokens.
__device__ void write_prefix_code(Strip &S, const u32 *hist, int nsym, u8 *len, u16 *code) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid == 0) {
    int used = 0, only = 0;
    for (int s = nsym - 1; s >= 0; --s)
      if (hist[s]) { ++used; only = s; }
    S.used = used;
    S.only = only;
  }
  __syncthreads();
  if (S.used < 2 && (S.used == 0 || S.only < 256)) {         // (the same for every thread)
    for (int s = tid; s < nsym; s += 256) { len[s] = 0; code[s] = 0; }
    if (tid == 0) put_simple_code(S, S.only);
    __syncthreads();
    return;
  }
  for (int s = tid; s < nsym; s += 256) S.B.cnt[s] = hist[s];
  build_lengths(S.B, nsym, 15, len);
  canonical_codes(S.B, nsym, len, code);
  if (tid < NCL) S.B.cnt[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    S.nseq = 0;
    run_length_form(S.seq, S.nseq, S.B.cnt, len, nsym);
  }
  build_lengths(S.B, NCL, 7, S.cl_len);
  canonical_codes(S.B, NCL, S.cl_len, S.cl_code);
  if (tid == 0) {
    int ncl = NCL;
    while (ncl > 4 && S.cl_len[CL_ORDER[ncl - 1]] == 0) --ncl;
    put_bits(S, 0, 1);
    put_bits(S, (u32)(ncl - 4), 4);
    for (int i = 0; i < ncl; ++i) put_bits(S, S.cl_len[CL_ORDER[i]], 3);
    put_bits(S, 0, 1);                                       // max_symbol: the whole alphabet
    for (int i = 0; i < S.nseq; ++i) {
      const int sym = S.seq[i] & 31, value = S.seq[i] >> 5;
      put_bits(S, S.cl_code[sym], S.cl_len[sym]);
      put_bits(S, (u32)value, sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
    }
  }
  __syncthreads();
}

// Every thread.  The image's `total` pixels as five prefix codes and their tokens, behind the S.at bits that one thread has put
// into the zeroed S.obuf.  split: the codes go to dst_head (bits in head_bits) and the tokens to dst from bit 0; else all goes
// to dst.  alpha is the one alpha value of the image.  -> the bits in dst.
template <class Src>
__device__ int code_image(Strip &S, const Src &src, int total, int alpha, bool split, u32 *__restrict__ dst_head, int &head_bits,
                          u32 *__restrict__ dst) {
  const int tid = threadIdx.x;
  for (int i = tid; i < NSYM; i += 256) S.hist_g[i] = 0;
  S.hist_r[tid] = 0;
  S.hist_b[tid] = 0;
  if (tid == 0) S.run_carry = -1;
  __syncthreads();

  // ---- first pass: the counts
  bool copies = false;
  for (int c0 = 0; c0 < total; c0 += CHUNK) {
    load_chunk(S, src, c0, total);
    int tok[PER];
    u32 val[PER];
    chunk_tokens(S, src, c0, total, tok, val);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (tok[i] > 0) {
        atomicAdd(&S.hist_g[256 + (length_prefix(tok[i]) & 255u)], 1u);
        copies = true;
      } else if (tok[i] == 0) {
        atomicAdd(&S.hist_g[(val[i] >> 8) & 255u], 1u);
        atomicAdd(&S.hist_r[(val[i] >> 16) & 255u], 1u);
        atomicAdd(&S.hist_b[val[i] & 255u], 1u);
      }
    }
  }
  const int any_copy = __syncthreads_or(copies ? 1 : 0);

  // ---- the five codes: green, red, blue, alpha, distance (a copy's distance 1 is plane code 2, prefix symbol 1)
  write_prefix_code(S, S.hist_g, NSYM, S.len_g, S.code_g);
  write_prefix_code(S, S.hist_r, 256, S.len_r, S.code_r);
  write_prefix_code(S, S.hist_b, 256, S.len_b, S.code_b);
  if (tid == 0) {
    put_simple_code(S, alpha);
    put_simple_code(S, any_copy ? 1 : 0);
    S.run_carry = -1;
  }
  __syncthreads();
  int running = S.at, wbase = 0;                             // bits so far; the word of dst that obuf[0] is
  if (split) {
    head_bits = running;
    const int words = (running + 31) >> 5;
    for (int k = tid; k < words; k += 256) dst_head[k] = S.obuf[k];
    __syncthreads();
    for (int k = tid; k < words; k += 256) S.obuf[k] = 0;
    running = 0;
    __syncthreads();
  }

  // ---- second pass: the tokens' bits
  for (int c0 = 0; c0 < total; c0 += CHUNK) {
    load_chunk(S, src, c0, total);
    int tok[PER];
    u32 val[PER];
    chunk_tokens(S, src, c0, total, tok, val);
    u64 word[PER];
    u8 wid[PER];
    int mine = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      u64 bits = 0;
      int width = 0;
      if (tok[i] > 0) {
        const u32 e = length_prefix(tok[i]);
        const int sym = 256 + (int)(e & 255u);
        width = S.len_g[sym];
        bits = (u64)S.code_g[sym] | ((u64)(e >> 16) << width);
        width += (int)((e >> 8) & 255u);                     // (the distance's code has one symbol: no bits)
      } else if (tok[i] == 0) {
        const int g = (val[i] >> 8) & 255u, r = (val[i] >> 16) & 255u, b = val[i] & 255u;
        bits = S.code_g[g];
        width = S.len_g[g];
        bits |= (u64)S.code_r[r] << width;
        width += S.len_r[r];
        bits |= (u64)S.code_b[b] << width;
        width += S.len_b[b];                                 // (alpha's code has one symbol: no bits)
      }
      word[i] = bits;
      wid[i] = (u8)width;
      mine += width;
    }
    int all;
    int at = running + block_exclusive_sum(S.wave_val, mine, all);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int width = wid[i];
      if (width) {
        const int k = (at >> 5) - wbase, sh = at & 31;
        const u64 rest = sh ? word[i] >> (32 - sh) : word[i] >> 32;
        atomicOr(&S.obuf[k], (u32)(word[i] << sh));
        if (sh + width > 32) atomicOr(&S.obuf[k + 1], (u32)rest);
        if (sh + width > 64) atomicOr(&S.obuf[k + 2], (u32)(rest >> 32));
        at += width;
      }
    }
    running += all;
    __syncthreads();
    const int full = (running >> 5) - wbase;
    for (int k = tid; k < full; k += 256) dst[wbase + k] = S.obuf[k];
    const u32 part = S.obuf[full];
    __syncthreads();
    for (int k = tid; k <= full + 2 && k < OWORDS; k += 256) S.obuf[k] = 0;
    __syncthreads();
    if (tid == 0) S.obuf[0] = part;
    wbase += full;
    __syncthreads();
  }
  const int words = ((running + 31) >> 5) - wbase;
  for (int k = tid; k < words; k += 256) dst[wbase + k] = S.obuf[k];
  return running;
}

// ---------------------------------------------------------------------------------------------- layout of the scratch
struct WebpLayout {
  int rows, groups, segs, bh, bw, across;
  int64_t slot0, slot1, head_slot, pixel_slot, frame_stage;  // bytes
  size_t ints, stage, total;
};

int64_t slot_bytes(int64_t bits) { return ((bits + 31) / 32 + 2) * 4; }       // whole words, two to spare

// ws: the two sums per frame (u64) | bits and bit offsets per segment | per frame the staging slots of its segments
bool webp_layout(int n, int h, int w, int pred_bits, int group_bits, WebpLayout &L) {
  if (n <= 0 || !webp_dims_ok(h, w) || !webp_bits_ok(pred_bits, group_bits)) return false;
  const int bs = 1 << pred_bits;
  L.bh = (h + bs - 1) / bs;
  L.bw = (w + bs - 1) / bs;
  L.rows = group_bits ? 1 << group_bits : h;
  L.groups = (h + L.rows - 1) / L.rows;
  L.across = group_bits ? (w + L.rows - 1) / L.rows : 0;
  L.segs = 2 + 2 * L.groups;
  L.slot0 = slot_bytes(PREAMBLE_BITS_MAX + SUB_HEADER_MAX + (int64_t)SUB_PIXEL_BITS_MAX * L.bh * L.bw);
  L.slot1 = slot_bytes(PREAMBLE_BITS_MAX + SUB_HEADER_MAX + (int64_t)SUB_PIXEL_BITS_MAX * L.groups * L.across);
  L.head_slot = slot_bytes(GROUP_HEADER_MAX);
  L.pixel_slot = slot_bytes((int64_t)MAIN_PIXEL_BITS_MAX * (L.rows < h ? L.rows : h) * w);
  L.frame_stage = L.slot0 + L.slot1 + L.groups * (L.head_slot + L.pixel_slot);
  L.ints = align256(sizeof(u64) * 2 * (size_t)n);
  L.stage = L.ints + align256(sizeof(int) * 2 * (size_t)n * L.segs);
  L.total = L.stage + (size_t)n * (size_t)L.frame_stage;
  return true;
}

__device__ __forceinline__ u32 *segment(u8 *stage, const WebpLayout &L, int64_t f, int k) {
  u8 *base = stage + f * L.frame_stage;
  if (k == 0) return (u32 *)base;
  if (k == 1) return (u32 *)(base + L.slot0);
  base += L.slot0 + L.slot1;
  if (k < 2 + L.groups) return (u32 *)(base + (int64_t)(k - 2) * L.head_slot);
  return (u32 *)(base + (int64_t)L.groups * L.head_slot + (int64_t)(k - 2 - L.groups) * L.pixel_slot);
}

// grid: one workgroup of 256 per (frame, strip)
__global__ __launch_bounds__(256) void webp_strip_kernel(const u32 *__restrict__ residual, int h, int w, WebpLayout L,
                                                         u8 *__restrict__ stage, int *__restrict__ bits_out) {
  __shared__ Strip S;
  const int tid = threadIdx.x;
  const int g = (int)(blockIdx.x % L.groups);
  const int64_t f = blockIdx.x / L.groups;
  const int rows = min(L.rows, h - g * L.rows);
  const int total = rows * w;                                // at most 2^24
  MainSrc src = {residual + (f * h + (int64_t)g * L.rows) * w};
  for (int i = tid; i < OWORDS; i += 256) S.obuf[i] = 0;
  if (tid == 0) S.at = 0;
  __syncthreads();
  int head_bits = 0;
  const int pixel_bits = code_image(S, src, total, 0, true, segment(stage, L, f, 2 + g), head_bits, segment(stage, L, f, 2 + L.groups + g));
  if (tid == 0) {
    bits_out[f * L.segs + 2 + g] = head_bits;
    bits_out[f * L.segs + 2 + L.groups + g] = pixel_bits;
  }
}

// grid: two workgroups of 256 per frame: the stream's head with the mode image; the main image's head with the entropy image
__global__ __launch_bounds__(256) void webp_head_kernel(const u8 *__restrict__ modes, const int *__restrict__ flags, int h, int w,
                                                        int pred_bits, int group_bits, WebpLayout L, u8 *__restrict__ stage,
                                                        int *__restrict__ bits_out) {
  __shared__ Strip S;
  const int tid = threadIdx.x;
  const int k = (int)(blockIdx.x & 1);
  const int64_t f = blockIdx.x >> 1;
  for (int i = tid; i < OWORDS; i += 256) S.obuf[i] = 0;
  if (tid == 0) S.at = 0;
  __syncthreads();
  u32 *dst = segment(stage, L, f, k);
  int unused = 0, bits;
  if (k == 0) {
    if (tid == 0) {
      put_bits(S, 0x2f, 8);
      put_bits(S, (u32)(w - 1), 14);
      put_bits(S, (u32)(h - 1), 14);
      put_bits(S, 0, 1);                                     // no alpha
      put_bits(S, 0, 3);                                     // version
      if (flags[f]) { put_bits(S, 1, 1); put_bits(S, 2, 2); }   // subtract green
      put_bits(S, 1, 1);
      put_bits(S, 0, 2);                                     // predictor transform
      put_bits(S, (u32)(pred_bits - 2), 3);
      put_bits(S, 0, 1);                                     // the mode image: no colour cache
    }
    __syncthreads();
    ModeSrc src = {modes + f * L.bh * L.bw};
    bits = code_image(S, src, L.bh * L.bw, 255, false, dst, unused, dst);
  } else {
    if (tid == 0) {
      put_bits(S, 0, 1);                                     // no more transforms
      put_bits(S, 0, 1);                                     // no colour cache
      put_bits(S, group_bits ? 1 : 0, 1);                    // the entropy image
      if (group_bits) {
        put_bits(S, (u32)(group_bits - 2), 3);
        put_bits(S, 0, 1);                                   // its own colour cache: none
      }
    }
    __syncthreads();
    if (group_bits) {
      GroupSrc src = {L.across};
      bits = code_image(S, src, L.groups * L.across, 255, false, dst, unused, dst);
    } else {
      bits = S.at;
      if (tid == 0) dst[0] = S.obuf[0];
    }
  }
  if (tid == 0) bits_out[f * L.segs + k] = bits;
}

// offs[f][k] = bits before segment k; out_len
__global__ __launch_bounds__(256) void webp_scan_kernel(const int *__restrict__ bits, int segs, int *__restrict__ offs,
                                                        int *__restrict__ out_len) {
  __shared__ int wave_tot[4];
  const int64_t f = blockIdx.x;
  const int running = carried_exclusive_sum(
      wave_tot, segs, 0, [&](int k) { return bits[f * segs + k]; }, [&](int k, int before) { offs[f * segs + k] = before; });
  if (threadIdx.x == 0) out_len[f] = (running + 7) >> 3;
}

// grid: one workgroup of 256 per (frame, segment)
__global__ __launch_bounds__(256) void webp_place_kernel(u8 *__restrict__ stage, WebpLayout L, const int *__restrict__ bits,
                                                         const int *__restrict__ offs, u8 *__restrict__ out, int64_t cap) {
  const int k = (int)(blockIdx.x % L.segs);
  const int64_t f = blockIdx.x / L.segs;
  const int *fbits = bits + f * L.segs;
  const int start = offs[f * L.segs + k], len = fbits[k];
  const u32 *own = segment(stage, L, f, k);
  u8 *dst = out + f * cap;
  const int j1 = (start + len - 1) >> 3;                     // (no byte starts in an empty segment: j1 is below the first j)
  for (int j = ((start + 7) >> 3) + threadIdx.x; j <= j1; j += 256) {
    const int p = 8 * j - start;
    int have = len - p;
    u32 v = bits8(own, p);
    if (have < 8) {                                          // the stream's last byte, or one that following segments fill
      v &= (1u << have) - 1;
      for (int kk = k + 1; kk < L.segs && have < 8; ++kk) {
        const int more = fbits[kk];
        if (more == 0) continue;
        const int take = min(more, 8 - have);
        v |= (segment(stage, L, f, kk)[0] & ((1u << take) - 1)) << have;
        have += take;
      }
    }
    dst[j] = (u8)v;
  }
}

int64_t frame_bits_max(int h, int w, int pred_bits, int group_bits) {
  const int64_t bs = 1 << pred_bits, bh = (h + bs - 1) / bs, bw = (w + bs - 1) / bs;
  int64_t bits = 40 + 3 + 6 + 1 + SUB_HEADER_MAX + SUB_PIXEL_BITS_MAX * bh * bw + 3, groups = 1;
  if (group_bits) {
    const int64_t rows = 1 << group_bits;
    groups = (h + rows - 1) / rows;
    bits += 3 + 1 + SUB_HEADER_MAX + SUB_PIXEL_BITS_MAX * groups * ((w + rows - 1) / rows);
  }
  return bits + groups * GROUP_HEADER_MAX + (int64_t)MAIN_PIXEL_BITS_MAX * h * w;
}

}  // namespace

extern "C" size_t sp_webp_ws_bytes(int n, int h, int w, int pred_bits, int group_bits) {
  WebpLayout L;
  return webp_layout(n, h, w, pred_bits, group_bits, L) ? L.total : 0;
}

// The derivation is in include/svdpipe.h; tests/webp_model.py stream_bound restates it.
extern "C" size_t sp_webp_stream_bytes(int h, int w, int pred_bits, int group_bits) {
  if (!webp_dims_ok(h, w) || !webp_bits_ok(pred_bits, group_bits)) return 0;
  return (size_t)((frame_bits_max(h, w, pred_bits, group_bits) + 7) / 8);
}

extern "C" int sp_webp_transform_u8(const void *frames, int n, int h, int w, int pred_bits, void *residual, void *modes, void *flags,
                                    void *ws, size_t ws_bytes, void *stream) {
  SP_REQUIRE(frames && residual && modes && flags && ws, "sp_webp_transform_u8: null pointer");
  SP_REQUIRE(n > 0 && webp_dims_ok(h, w), "sp_webp_transform_u8: n must be positive, h and w in 1..16384 and h*w <= 2^24 (n=%d, %dx%d)",
             n, h, w);
  SP_REQUIRE(pred_bits >= 2 && pred_bits <= 9, "sp_webp_transform_u8: pred_bits %d is not in 2..9", pred_bits);
  SP_REQUIRE(ws_bytes >= sizeof(u64) * 2 * (size_t)n, "sp_webp_transform_u8: ws holds %zu bytes, needs %zu", ws_bytes,
             sizeof(u64) * 2 * (size_t)n);
  SP_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)flags % 4 == 0 && (uintptr_t)residual % 4 == 0,
             "sp_webp_transform_u8: ws must be 8-byte, flags and residual 4-byte aligned");
  const int bs = 1 << pred_bits, bh = (h + bs - 1) / bs, bw = (w + bs - 1) / bs;
  const int64_t rows = (int64_t)n * h, block_rows = (int64_t)n * bh;
  SP_REQUIRE(rows <= 0x7fffffff, "sp_webp_transform_u8: too many rows (%lld)", (long long)rows);
  hipStream_t s = (hipStream_t)stream;
  SP_CLEAR_STALE_ERROR();
  if (hipMemsetAsync(ws, 0, sizeof(u64) * 2 * (size_t)n, s) != hipSuccess) {
    sp_set_error("sp_webp_transform_u8: clearing the sums failed");
    return SP_ELAUNCH;
  }
  hipLaunchKernelGGL(webp_cost_kernel, dim3((unsigned)rows), dim3(256), 0, s, (const u8 *)frames, h, w, (u64 *)ws);
  hipLaunchKernelGGL(webp_transform_kernel, dim3((unsigned)block_rows), dim3(256), 0, s, (const u8 *)frames, h, w, pred_bits, bh, bw,
                     (const u64 *)ws, (int *)flags, (u8 *)modes, (u32 *)residual);
  SP_CHECK_LAUNCH("sp_webp_transform_u8");
  return SP_OK;
}

extern "C" int sp_webp_code(const void *residual, const void *modes, const void *flags, int n, int h, int w, int pred_bits,
                            int group_bits, void *out, size_t cap, void *out_len, void *ws, size_t ws_bytes, void *stream) {
  SP_REQUIRE(residual && modes && flags && out && out_len && ws, "sp_webp_code: null pointer");
  SP_REQUIRE(n > 0 && webp_dims_ok(h, w), "sp_webp_code: n must be positive, h and w in 1..16384 and h*w <= 2^24 (n=%d, %dx%d)", n, h, w);
  SP_REQUIRE(webp_bits_ok(pred_bits, group_bits), "sp_webp_code: pred_bits must be 2..9 and group_bits 0 or 2..9 (%d, %d)", pred_bits,
             group_bits);
  WebpLayout L;
  webp_layout(n, h, w, pred_bits, group_bits, L);
  const size_t need = sp_webp_stream_bytes(h, w, pred_bits, group_bits);
  SP_REQUIRE(cap >= need, "sp_webp_code: cap is %zu bytes per frame, a frame can need %zu (sp_webp_stream_bytes)", cap, need);
  SP_REQUIRE(ws_bytes >= L.total, "sp_webp_code: ws holds %zu bytes, needs %zu (sp_webp_ws_bytes)", ws_bytes, L.total);
  SP_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)out_len % 4 == 0 && (uintptr_t)flags % 4 == 0 && (uintptr_t)residual % 4 == 0,
             "sp_webp_code: ws must be 8-byte, out_len, flags and residual 4-byte aligned");
  const int64_t strips = (int64_t)n * L.groups, segs = (int64_t)n * L.segs;
  SP_REQUIRE(segs <= 0x7fffffff, "sp_webp_code: too many segments (%lld)", (long long)segs);
  hipStream_t s = (hipStream_t)stream;
  u8 *base = (u8 *)ws;
  int *bits = (int *)(base + L.ints), *offs = bits + segs;
  u8 *stage = base + L.stage;
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(webp_strip_kernel, dim3((unsigned)strips), dim3(256), 0, s, (const u32 *)residual, h, w, L, stage, bits);
  hipLaunchKernelGGL(webp_head_kernel, dim3((unsigned)(2 * n)), dim3(256), 0, s, (const u8 *)modes, (const int *)flags, h, w, pred_bits,
                     group_bits, L, stage, bits);
  hipLaunchKernelGGL(webp_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, (const int *)bits, L.segs, offs, (int *)out_len);
  hipLaunchKernelGGL(webp_place_kernel, dim3((unsigned)segs), dim3(256), 0, s, stage, L, (const int *)bits, (const int *)offs, (u8 *)out,
                     (int64_t)cap);
  SP_CHECK_LAUNCH("sp_webp_code");
  return SP_OK;
}
