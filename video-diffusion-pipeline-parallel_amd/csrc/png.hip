// PNG / APNG frames of uint8 frames that are already in device memory: the lossless output of save_frames.  The library makes,
// per frame, the filtered rows and the complete zlib stream of them, and then the files around the streams: one still per
// frame or one animation, byte for byte what models/image_io.py png_file / write_apng build on the host (which remain the
// statement the device files are held to).  include/svdpipe.h fixes the rules, tests/png_model.py restates them.
//
//   png_filter_kernel  : a workgroup per row: the five sums of min(b, 256 - b), the choice, then the chosen row (bytes: the
//                        pitch 1 + 3w is rarely aligned).
//   png_deflate_kernel : a workgroup per (frame, strip), one dynamic-Huffman block.  The strip passes through LDS twice in
//                        chunks of 4096 bytes, 16 consecutive bytes per thread.  A position's token follows from the start of
//                        its run of equal bytes (a max-scan over the threads, carried from chunk to chunk) and from at most 257
//                        bytes ahead (the chunk has that halo): at distance k >= 1 from the run's start, j = k - 1, a token
//                        starts where j % 258 == 0 (a match of the bytes ahead, capped at 258, if they are at least 3, else a
//                        literal) and where j % 258 == 1 and the run ends here (the second literal of a remainder of 2).
//                        First pass: histogram by LDS atomics and the Adler-32 partials.  Then the code (codec_common.h):
//                        a rank sort by (count, symbol) by all threads, the two-queue merge and the depths by one thread (at
//                        most 285 joins), the halving loop around both; canonical codes; the run-length form of the lengths
//                        and the 19-symbol code by the same builder; the header bits by one thread.  Second pass: bits per
//                        token, a prefix sum, and every token ORed into an LDS image of the chunk's words, which then goes to the strip's staging
//                        slot in whole words.
//   png_scan_kernel    : per frame the exclusive sum of the strips' bit counts, the byte count, 78 9C in front, the Adler-32
//                        folded from the strips' partials behind, out_len.
//   png_place_kernel   : one workgroup per strip writes the bytes whose first bit lies in the strip (gif_place_kernel's rule).
//   png_head_kernel    : one workgroup, a thread per frame: the exclusive sum of the chunk sizes (an animation's frames follow
//                        one another), and every byte of the files that is no stream and no stream's CRC: signature, IHDR,
//                        acTL, fcTL, the length and type of IDAT / fdAT and an fdAT's sequence number, IEND, each small chunk's
//                        CRC bit by bit; the CRC-32 of a data chunk's type (and sequence number) as the seed of its stream's.
//   (crc32.hip)        : the CRC-32 of every stream from that seed, parallel within a stream.
//   png_copy_kernel    : a workgroup per 16 KiB of a stream: the stream to its place in whole words of the destination, the
//                        CRC behind it.
// Nothing here is tuned beyond its layout; profiles/png_timing.txt has what it costs.
#include "codec_common.h"

namespace {

constexpr int MAX_PIXELS = 1 << 24;
constexpr int NSYM = 286, NCL = 19, END_OF_BLOCK = 256;
constexpr int HEADER_BITS_MAX = 3 + 14 + 19 * 3 + (286 + 2) * 14;
constexpr int TOKEN_BITS_MAX = 15;
constexpr int CHUNK = 4096, PER = 16, HALO = 260;
constexpr int OWORDS = 2064;             // header + one chunk's tokens + the end-of-block: (4106 + 4095 * 15 + 21 + 15 + 31) / 32 < 2056
constexpr u32 ADLER = 65521;

__constant__ u16 LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ u8 LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ u8 CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

bool png_dims_ok(int h, int w) { return h > 0 && w > 0 && h <= 65535 && w <= 65535 && (int64_t)h * w <= MAX_PIXELS; }

// ---------------------------------------------------------------------------------------------- filter
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// grid: one workgroup of 256 per row of every frame
__global__ __launch_bounds__(256) void png_filter_kernel(const u8 *__restrict__ frames, int h, int w, u8 *__restrict__ filtered) {
  __shared__ u32 red[4][5];
  __shared__ int chosen;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t row = blockIdx.x;
  const bool top = row % h == 0;
  const int n = 3 * w;
  const u8 *cur = frames + row * n, *up = cur - n;         // (up is read only below the top row)
  u8 *dst = filtered + row * ((int64_t)n + 1);
  u32 s[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += 256) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = top ? 0 : up[i], c = (top || i < 3) ? 0 : up[i - 3];
    s[0] += byte_cost(x);
    s[1] += byte_cost(x - a);
    s[2] += byte_cost(x - b);
    s[3] += byte_cost(x - ((a + b) >> 1));
    s[4] += byte_cost(x - paeth(a, b, c));
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
    if (lane == 0) red[wv][k] = s[k];
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    u32 best_sum = 0xffffffffu;
    for (int k = 0; k < 5; ++k) {
      const u32 v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
      if (v < best_sum) { best_sum = v; best = k; }         // (strictly less: the lower type among equals)
    }
    chosen = best;
    dst[0] = (u8)best;
  }
  __syncthreads();
  const int t = chosen;
  for (int i = tid; i < n; i += 256) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = top ? 0 : up[i], c = (top || i < 3) ? 0 : up[i - 3];
    const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? ((a + b) >> 1) : paeth(a, b, c);
    dst[1 + i] = (u8)(x - pred);
  }
}

// ---------------------------------------------------------------------------------------------- the strip
// (the code construction, HuffBuilder and what works on it, is in codec_common.h)
struct Strip {
  __align__(16) u8 buf[16 + CHUNK + HALO + 12];   // [15]: the byte before the chunk; [16 ..): the chunk and its halo
  u32 obuf[OWORDS];
  HuffBuilder<NSYM> B;
  u32 lentab[256];                      // match length - 3 -> length code index | extra bits << 8 | extra value << 16
  u8 len[NSYM];
  u16 code[NSYM];
  u8 cl_len[NCL];
  u16 cl_code[NCL];
  u16 seq[NSYM + 2];                    // the run-length form: symbol | extra value << 5
  int nseq, nlit, header_bits;
  int wave_val[4];
  int run_carry;
  u64 adler_a, adler_b;
};

__device__ __forceinline__ void load_chunk(Strip &S, const u8 *__restrict__ src, int c0, int total) {
  __syncthreads();
  for (int i = threadIdx.x; i < CHUNK + HALO + 1; i += 256) {
    const int q = c0 - 1 + i;
    S.buf[15 + i] = (q >= 0 && q < total) ? src[q] : (u8)0;
  }
  __syncthreads();
}

// tok[i] for the thread's positions c0 + 16 tid + i: -1 none, 0 .. 255 a literal, 256 + length a match
__device__ __forceinline__ void chunk_tokens(Strip &S, int c0, int total, int (&tok)[PER], u8 (&val)[PER]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p0 = c0 + tid * PER;
  const u32 *wp = (const u32 *)(S.buf + 12 + tid * PER);
  u32 wd[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) wd[k] = wp[k];
  auto byte_at = [&](int j) -> int { return (int)((wd[(j + 4) >> 2] >> (8 * ((j + 4) & 3))) & 255u); };   // j = -4 .. 19
  u32 flags = 0;
  int last = -1;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int p = p0 + i;
    val[i] = (u8)byte_at(i);
    if (p < total && (p == 0 || byte_at(i) != byte_at(i - 1))) { flags |= 1u << i; last = p; }
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
    const int v = byte_at(i);
    if (flags & (1u << i)) { start = p; tok[i] = v; continue; }
    const int jm = (p - start - 1) % 258;
    if (jm == 0) {
      const bool three = p + 2 < total && byte_at(i + 1) == v && byte_at(i + 2) == v;
      if (!three) tok[i] = v;
      else {
        const int lim = min(258, total - p);
        const u8 *ahead = S.buf + 16 + tid * PER + i;
        int r = 3;
        while (r < lim && ahead[r] == v) ++r;
        tok[i] = 256 + r;
      }
    } else if (jm == 1) {
      if (p + 1 >= total || byte_at(i + 1) != v) tok[i] = v;
    }
  }
}

// grid: one workgroup of 256 per (frame, strip)
__global__ __launch_bounds__(256) void png_deflate_kernel(const u8 *__restrict__ filtered, int h, int pitch, int strip_rows, int strips,
                                                          u8 *__restrict__ stage, int64_t slot_bytes, int *__restrict__ bits_out,
                                                          u32 *__restrict__ adler_out) {
  __shared__ Strip S;
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int s = (int)(bid % strips);
  const int64_t f = bid / strips;
  const int rows = min(strip_rows, h - s * strip_rows);
  const int total = rows * pitch;                            // at most 2^24 * 3 + 65535 bytes
  const u8 *src = filtered + (f * h + (int64_t)s * strip_rows) * pitch;
  u32 *dst = (u32 *)(stage + bid * slot_bytes);

  for (int i = tid; i < NSYM; i += 256) S.B.cnt[i] = 0;
  {
    const int l = tid + 3;                                   // 3 .. 258
    int k = 28;
    while (LEN_BASE[k] > l) --k;
    S.lentab[tid] = (u32)k | ((u32)LEN_EXTRA[k] << 8) | ((u32)(l - LEN_BASE[k]) << 16);
  }
  if (tid == 0) { S.run_carry = -1; S.adler_a = 0; S.adler_b = 0; }
  __syncthreads();

  // ---- first pass: the counts and the Adler-32 partials
  u64 sum_a = 0, sum_b = 0;
  for (int c0 = 0; c0 < total; c0 += CHUNK) {
    load_chunk(S, src, c0, total);
    int tok[PER];
    u8 val[PER];
    chunk_tokens(S, c0, total, tok, val);
    const int p0 = c0 + tid * PER;
    u32 a = 0, weighted = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (tok[i] >= 256) atomicAdd(&S.B.cnt[257 + (S.lentab[tok[i] - 259] & 255u)], 1u);
      else if (tok[i] >= 0) atomicAdd(&S.B.cnt[tok[i]], 1u);
      if (p0 + i < total) { a += val[i]; weighted += (u32)i * val[i]; }
    }
    if (p0 < total) {                                        // the byte at p counts total - p times in B
      sum_a += a;
      sum_b += (u64)(total - p0) * a - weighted;
    }
  }
  atomicAdd(&S.adler_a, sum_a);
  atomicAdd(&S.adler_b, sum_b);
  __syncthreads();
  if (tid == 0) {
    S.B.cnt[END_OF_BLOCK] = 1;
    adler_out[2 * bid] = (u32)(S.adler_a % ADLER);
    adler_out[2 * bid + 1] = (u32)(S.adler_b % ADLER);
  }

  // ---- the two codes and the block header
  build_lengths(S.B, NSYM, 15, S.len);
  canonical_codes(S.B, NSYM, S.len, S.code);
  for (int i = tid; i < OWORDS; i += 256) S.obuf[i] = 0;
  if (tid < NCL) S.B.cnt[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    int nlit = NSYM;
    while (S.len[nlit - 1] == 0) --nlit;                     // (>= 257: end-of-block has a code)
    S.nlit = nlit;
    S.nseq = 0;
    run_length_form(S.seq, S.nseq, S.B.cnt, S.len, nlit);
    S.seq[S.nseq++] = 1; S.seq[S.nseq++] = 1;               // the distance code: two lengths of 1, too few for a repeat
    S.B.cnt[1] += 2;
  }
  build_lengths(S.B, NCL, 7, S.cl_len);
  canonical_codes(S.B, NCL, S.cl_len, S.cl_code);
  if (tid == 0) {
    int at = 0;
    auto put = [&](u32 value, int width) { put_bits(S.obuf, at, value, width); };
    int ncl = NCL;
    while (ncl > 4 && S.cl_len[CL_ORDER[ncl - 1]] == 0) --ncl;
    put(s + 1 == strips ? 1u : 0u, 1);
    put(2, 2);
    put((u32)(S.nlit - 257), 5);
    put(1, 5);
    put((u32)(ncl - 4), 4);
    for (int i = 0; i < ncl; ++i) put(S.cl_len[CL_ORDER[i]], 3);
    for (int i = 0; i < S.nseq; ++i) {
      const int sym = S.seq[i] & 31, value = S.seq[i] >> 5;
      put(S.cl_code[sym], S.cl_len[sym]);
      put((u32)value, sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
    }
    S.header_bits = at;
    S.run_carry = -1;
  }
  __syncthreads();

  // ---- second pass: the tokens' bits
  int running = S.header_bits, wbase = 0;                    // bits so far; the word of the stream that obuf[0] is
  for (int c0 = 0; c0 < total; c0 += CHUNK) {
    load_chunk(S, src, c0, total);
    int tok[PER];
    u8 val[PER];
    chunk_tokens(S, c0, total, tok, val);
    u32 word[PER];                                           // bits | width << 24
    int mine = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      u32 bits = 0;
      int width = 0;
      if (tok[i] >= 256) {
        const u32 e = S.lentab[tok[i] - 259];
        const int sym = 257 + (int)(e & 255u), extra = (int)((e >> 8) & 255u);
        width = S.len[sym];
        bits = (u32)S.code[sym] | ((e >> 16) << width);
        width += extra + 1;                                  // and distance 1: the one-bit code 0
      } else if (tok[i] >= 0) {
        width = S.len[tok[i]];
        bits = S.code[tok[i]];
      }
      word[i] = bits | ((u32)width << 24);
      mine += width;
    }
    int all;
    int at = running + block_exclusive_sum(S.wave_val, mine, all);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int width = (int)(word[i] >> 24);
      if (width) {
        const u32 bits = word[i] & 0xffffffu;
        const int k = (at >> 5) - wbase, sh = at & 31;
        atomicOr(&S.obuf[k], bits << sh);
        if (sh + width > 32) atomicOr(&S.obuf[k + 1], bits >> (32 - sh));
        at += width;
      }
    }
    running += all;
    __syncthreads();
    const int full = (running >> 5) - wbase;
    for (int k = tid; k < full; k += 256) dst[wbase + k] = S.obuf[k];
    const u32 part = S.obuf[full];
    __syncthreads();
    for (int k = tid; k <= full + 1 && k < OWORDS; k += 256) S.obuf[k] = 0;
    __syncthreads();
    if (tid == 0) S.obuf[0] = part;
    wbase += full;
    __syncthreads();
  }
  if (tid == 0) {
    int at = running - 32 * wbase;                           // (obuf[0] is word wbase of the stream)
    put_bits(S.obuf, at, S.code[END_OF_BLOCK], S.len[END_OF_BLOCK]);
    bits_out[bid] = running + S.len[END_OF_BLOCK];
  }
  running += S.len[END_OF_BLOCK];
  __syncthreads();
  const int words = ((running + 31) >> 5) - wbase;
  for (int k = tid; k < words; k += 256) dst[wbase + k] = S.obuf[k];
}

// offs[f][k] = bits before strip k; data_bytes[f]; 78 9C in front, the Adler-32 behind, out_len
__global__ __launch_bounds__(256) void png_scan_kernel(const int *__restrict__ bits, const u32 *__restrict__ adler, int h, int pitch,
                                                       int strip_rows, int strips, int *__restrict__ offs, int *__restrict__ data_bytes,
                                                       u8 *__restrict__ out, int64_t cap, int *__restrict__ out_len) {
  __shared__ int wave_tot[4];
  __shared__ u64 fold_a, fold_b;
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x;
  const int64_t whole = (int64_t)h * pitch;
  if (tid == 0) { fold_a = 0; fold_b = 0; }
  u64 a_sum = 0, b_sum = 0;
  const int running = carried_exclusive_sum(
      wave_tot, strips, 0, [&](int k) { return bits[f * strips + k]; },
      [&](int k, int before) {
        offs[f * strips + k] = before;
        // a byte of strip k counts, beyond its place in the strip, once per byte behind the strip
        const int64_t behind = whole - min((int64_t)h, ((int64_t)k + 1) * strip_rows) * pitch;
        const u64 a = adler[2 * (f * strips + k)], b = adler[2 * (f * strips + k) + 1];
        a_sum += a;
        b_sum += b + a * (u64)(behind % ADLER);
      });
  atomicAdd(&fold_a, a_sum);
  atomicAdd(&fold_b, b_sum);
  __syncthreads();
  if (tid == 0) {
    const int nbytes = (running + 7) >> 3;
    const u32 a = (u32)((1 + fold_a) % ADLER), b = (u32)(((u64)(whole % ADLER) + fold_b) % ADLER);
    u8 *dst = out + f * cap;
    data_bytes[f] = nbytes;
    dst[0] = 0x78; dst[1] = 0x9C;
    dst[2 + nbytes] = (u8)(b >> 8); dst[3 + nbytes] = (u8)b; dst[4 + nbytes] = (u8)(a >> 8); dst[5 + nbytes] = (u8)a;
    out_len[f] = 2 + nbytes + 4;
  }
}

// grid: one workgroup of 256 per (frame, strip)
__global__ __launch_bounds__(256) void png_place_kernel(const u8 *__restrict__ stage, int64_t slot_bytes, const int *__restrict__ bits,
                                                        const int *__restrict__ offs, int strips, u8 *__restrict__ out, int64_t cap) {
  const int64_t bid = blockIdx.x;
  const int s = (int)(bid % strips);
  const int64_t f = bid / strips;
  const int start = offs[bid], len = bits[bid];
  const u32 *own = (const u32 *)(stage + bid * slot_bytes);
  const u32 *next = (const u32 *)(stage + (bid + 1) * slot_bytes);
  u8 *dst = out + f * cap + 2;
  const int j1 = (start + len - 1) >> 3;
  for (int j = ((start + 7) >> 3) + threadIdx.x; j <= j1; j += 256) {
    const int p = 8 * j - start, avail = len - p;
    u32 v = bits8(own, p);
    if (avail < 8) {
      v &= (1u << avail) - 1;
      if (s + 1 < strips) v |= (next[0] << avail) & 255u;   // (a block is longer than 8 bits: its header alone has 17)
    }
    dst[j] = (u8)v;
  }
}

// ---------------------------------------------------------------------------------------------- files
constexpr int COPY_WORDS = 4096;        // words of a file that one workgroup of png_copy_kernel writes
constexpr int STILL_EXTRA = 57;         // signature 8, IHDR 25, IDAT 12 around its payload, IEND 12
constexpr int APNG_FIXED = 65;          // signature 8, IHDR 25, acTL 20, IEND 12
constexpr int APNG_FRAME = 50;          // fcTL 38, IDAT 12 around its payload; an fdAT has its sequence number, 4 more

__device__ __forceinline__ void put_be16(u8 *p, u32 v) { p[0] = (u8)(v >> 8); p[1] = (u8)v; }
__device__ __forceinline__ void put_be32(u8 *p, u32 v) { p[0] = (u8)(v >> 24); p[1] = (u8)(v >> 16); p[2] = (u8)(v >> 8); p[3] = (u8)v; }
// a chunk's length and type
__device__ __forceinline__ void put_head(u8 *p, u32 len, char a, char b, char c, char d) {
  put_be32(p, len);
  p[4] = (u8)a; p[5] = (u8)b; p[6] = (u8)c; p[7] = (u8)d;
}
// zlib.crc32 of a few bytes, bit by bit
__device__ u32 crc_small(const u8 *p, int n) {
  u32 r = 0xffffffffu;
  for (int i = 0; i < n; ++i) {
    r ^= p[i];
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
  }
  return ~r;
}
// the CRC behind the chunk at p, whose type and n bytes of payload this thread has written
__device__ __forceinline__ void seal(u8 *p, int n) { put_be32(p + 8 + n, crc_small(p + 4, 4 + n)); }

__device__ void put_front(u8 *p, int h, int w) {              // the signature and IHDR: 8 bits, RGB, no interlace
  const u8 sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  for (int i = 0; i < 8; ++i) p[i] = sig[i];
  p += 8;
  put_head(p, 13, 'I', 'H', 'D', 'R');
  put_be32(p + 8, (u32)w);
  put_be32(p + 12, (u32)h);
  p[16] = 8; p[17] = 2; p[18] = 0; p[19] = 0; p[20] = 0;
  seal(p, 13);
}
__device__ void put_iend(u8 *p) {
  put_head(p, 0, 'I', 'E', 'N', 'D');
  seal(p, 0);
}

// One workgroup of 256, a thread per frame: everything of the files but the streams and their CRCs.  where[i]: the place of
// frame i's stream in `files`; seed[i]: the CRC-32 of what the chunk's CRC covers in front of the stream (the type, and an
// fdAT's sequence number).  A length outside 0 .. cap counts as the nearer end, here and in the two kernels behind.
__global__ __launch_bounds__(256) void png_head_kernel(const int *__restrict__ lens, int n, int64_t cap, int h, int w, int animate,
                                                       int delay_num, int delay_den, u8 *files, int64_t file_cap, int *file_len,
                                                       int64_t *__restrict__ where, u32 *__restrict__ seed) {
  __shared__ int wave_tot[4];
  const int tid = threadIdx.x;
  const auto len_of = [&](int i) { return (int)min((int64_t)max(lens[i], 0), cap); };
  if (!animate) {                                            // (the whole workgroup)
    for (int i = tid; i < n; i += 256) {
      const int len = len_of(i);
      u8 *p = files + i * file_cap;
      put_front(p, h, w);
      put_head(p + 33, (u32)len, 'I', 'D', 'A', 'T');
      seed[i] = crc_small(p + 37, 4);
      where[i] = i * file_cap + 41;
      put_iend(p + 41 + len + 4);
      file_len[i] = len + STILL_EXTRA;
    }
    return;
  }
  // frame i's fcTL and the head of its IDAT / fdAT at `at`
  const auto put_frame = [&](int i, int at) {
    const int len = len_of(i);
    u8 *p = files + at;
    if (i == 0) {
      put_front(files, h, w);
      put_head(files + 33, 8, 'a', 'c', 'T', 'L');
      put_be32(files + 41, (u32)n);
      put_be32(files + 45, 0);                               // num_plays: for ever
      seal(files + 33, 8);
    }
    put_head(p, 26, 'f', 'c', 'T', 'L');
    put_be32(p + 8, i ? 2u * i - 1 : 0u);
    put_be32(p + 12, (u32)w);
    put_be32(p + 16, (u32)h);
    put_be32(p + 20, 0);
    put_be32(p + 24, 0);
    put_be16(p + 28, (u32)delay_num);
    put_be16(p + 30, (u32)delay_den);
    p[32] = 0; p[33] = 0;                                    // dispose none, blend source
    seal(p, 26);
    p += 38;
    if (i == 0) put_head(p, (u32)len, 'I', 'D', 'A', 'T');
    else {
      put_head(p, (u32)len + 4, 'f', 'd', 'A', 'T');
      put_be32(p + 8, 2u * i);
    }
    seed[i] = crc_small(p + 4, i ? 8 : 4);
    where[i] = (p - files) + (i ? 12 : 8);
  };
  // frame 0's fcTL starts behind acTL; the frames follow one another
  const int end = carried_exclusive_sum(
      wave_tot, n, APNG_FIXED - 12, [&](int i) { return APNG_FRAME + len_of(i) + (i ? 4 : 0); }, put_frame);
  if (tid == 0) {
    put_iend(files + end);
    file_len[0] = end + 12;
  }
}

// grid: frames * chunks workgroups of 256, chunks = ceil(cap / (4 COPY_WORDS)): frame i's stream to where[i] in whole words
// of the destination (the source comes through load_bytes4), its ends in bytes, and the chunk's CRC behind it
__global__ __launch_bounds__(256) void png_copy_kernel(const u8 *__restrict__ streams, int64_t cap, const int *__restrict__ lens,
                                                       int chunks, const int64_t *__restrict__ where, const u32 *__restrict__ crc,
                                                       u8 *__restrict__ files) {
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int j = (int)(bid % chunks);
  const int64_t i = bid / chunks;
  const int len = (int)min((int64_t)max(lens[i], 0), cap);
  const u8 *src = streams + i * cap;
  u8 *dst = files + where[i];
  const int head = min(len, (int)((0 - (uintptr_t)dst) & 3)), words = (len - head) >> 2, tail = len - head - 4 * words;
  if (j == 0) {
    if (tid < head) dst[tid] = src[tid];
    if (tid < tail) dst[head + 4 * words + tid] = src[head + 4 * words + tid];
    if (tid < 4) dst[len + tid] = (u8)(crc[i] >> (24 - 8 * tid));
  }
  u32 *body = (u32 *)(dst + head);
  const int k1 = min(words, (j + 1) * COPY_WORDS);
  for (int k = j * COPY_WORDS + tid; k < k1; k += 256) body[k] = load_bytes4(src, head + 4 * (int64_t)k, len);
}

struct PngLayout {
  int rows, strips, pitch;
  size_t ints, stage, total;
  int64_t slot;
};

// ws: bits, offsets (per strip), byte counts (per frame), Adler partials (two per strip) | staging slots
bool png_layout(int n, int h, int w, int strip_rows, PngLayout &L) {
  if (n <= 0 || !png_dims_ok(h, w) || strip_rows < 1) return false;
  L.rows = strip_rows < h ? strip_rows : h;
  L.strips = (h + L.rows - 1) / L.rows;
  L.pitch = 1 + 3 * w;
  const int64_t strip_bits = HEADER_BITS_MAX + (int64_t)TOKEN_BITS_MAX * L.rows * L.pitch + TOKEN_BITS_MAX;
  L.slot = ((strip_bits + 31) / 32 + 1) * 4;                 // whole words, one to spare
  L.ints = 0;
  L.stage = align256(sizeof(int) * ((size_t)4 * n * L.strips + n));
  L.total = L.stage + (size_t)n * L.strips * (size_t)L.slot;
  return true;
}

}  // namespace

extern "C" size_t sp_png_ws_bytes(int n, int h, int w, int strip_rows) {
  PngLayout L;
  return png_layout(n, h, w, strip_rows, L) ? L.total : 0;
}

// Bits of one frame: per strip a block header of at most 3 + 14 + 19*3 + (286 + 2) * 14 = 4106 bits (BFINAL and BTYPE; HLIT,
// HDIST, HCLEN; 19 lengths of 3 bits; a run-length symbol of at most 7 bits with at most 7 extra bits per code length) and an
// end-of-block code of at most 15 bits; at most one token per byte, a literal of at most 15 bits or a match of at most
// 15 + 5 + 1 bits that covers at least 3 bytes.  Rounded up to bytes, 78 9C in front and the Adler-32 behind.
extern "C" size_t sp_png_stream_bytes(int h, int w, int strip_rows) {
  if (!png_dims_ok(h, w) || strip_rows < 1) return 0;
  const int64_t rows = strip_rows < h ? strip_rows : h, strips = (h + rows - 1) / rows;
  const int64_t bits = strips * (HEADER_BITS_MAX + TOKEN_BITS_MAX) + (int64_t)TOKEN_BITS_MAX * h * (1 + 3 * (int64_t)w);
  return (size_t)(2 + (bits + 7) / 8 + 4);
}

extern "C" size_t sp_png_file_bytes(int h, int w, int strip_rows) {
  const size_t s = sp_png_stream_bytes(h, w, strip_rows);
  return s ? s + STILL_EXTRA : 0;
}

extern "C" size_t sp_apng_file_bytes(int n, int h, int w, int strip_rows) {
  const size_t s = sp_png_stream_bytes(h, w, strip_rows);
  return (s && n > 0) ? APNG_FIXED + (size_t)n * (APNG_FRAME + s) + 4 * ((size_t)n - 1) : 0;
}

// ws: where (int64 per frame), seeds and CRCs (uint32 per frame each) | the CRC's scratch
extern "C" size_t sp_png_wrap_ws_bytes(int n, size_t cap) {
  const size_t crc = sp_crc32_ws_bytes(n, cap);
  return crc ? align256((size_t)16 * n) + crc : 0;
}

extern "C" int sp_png_wrap(const void *streams, size_t cap, const void *lens, int n, int h, int w, int animate, int delay_num,
                           int delay_den, void *files, size_t file_cap, void *file_len, void *ws, size_t ws_bytes, void *stream) {
  SP_REQUIRE(streams && lens && files && file_len && ws, "sp_png_wrap: null pointer");
  SP_REQUIRE(n > 0 && png_dims_ok(h, w), "sp_png_wrap: n must be positive, h and w in 1..65535 and h*w <= 2^24 (n=%d, %dx%d)", n, h, w);
  SP_REQUIRE(cap > 0 && cap <= (size_t)0x7fffffff - STILL_EXTRA, "sp_png_wrap: cap %zu is not in 1..2^31-58", cap);
  const size_t need_file = animate ? APNG_FIXED + (size_t)n * (APNG_FRAME + cap) + 4 * ((size_t)n - 1) : cap + STILL_EXTRA;
  SP_REQUIRE(need_file <= (size_t)0x7fffffff, "sp_png_wrap: an animation of %d frames of %zu bytes does not fit an int32 length", n, cap);
  SP_REQUIRE(file_cap >= need_file, "sp_png_wrap: file_cap is %zu bytes, streams of cap %zu can need %zu (sp_png_file_bytes / sp_apng_file_bytes)",
             file_cap, cap, need_file);
  if (animate) {
    SP_REQUIRE(delay_num >= 1 && delay_num <= 65535 && delay_den >= 0 && delay_den <= 65535,
               "sp_png_wrap: the delay %d / %d does not fit fcTL's 16-bit fields (numerator 1..65535, denominator 0..65535)", delay_num,
               delay_den);
  }
  const size_t need = sp_png_wrap_ws_bytes(n, cap);
  SP_REQUIRE(ws_bytes >= need, "sp_png_wrap: ws holds %zu bytes, needs %zu (sp_png_wrap_ws_bytes)", ws_bytes, need);
  SP_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)lens % 4 == 0 && (uintptr_t)file_len % 4 == 0,
             "sp_png_wrap: ws must be 8-byte, lens and file_len 4-byte aligned");
  const int chunks = (int)((cap + 4 * (size_t)COPY_WORDS - 1) / (4 * (size_t)COPY_WORDS));
  SP_REQUIRE((int64_t)n * chunks <= 0x7fffffff && sp_crc32_ws_bytes(n, cap) / 4 <= (size_t)0x7fffffff, "sp_png_wrap: too many frames (%d)", n);
  hipStream_t s = (hipStream_t)stream;
  u8 *base = (u8 *)ws;
  int64_t *where = (int64_t *)base;
  u32 *seed = (u32 *)(where + n), *crc = seed + n;
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(png_head_kernel, dim3(1), dim3(256), 0, s, (const int *)lens, n, (int64_t)cap, h, w, animate, delay_num, delay_den,
                     (u8 *)files, (int64_t)file_cap, (int *)file_len, where, seed);
  sp_crc32_launch(streams, cap, lens, seed, n, crc, base + align256((size_t)16 * n), s);
  hipLaunchKernelGGL(png_copy_kernel, dim3((unsigned)((int64_t)n * chunks)), dim3(256), 0, s, (const u8 *)streams, (int64_t)cap,
                     (const int *)lens, chunks, (const int64_t *)where, (const u32 *)crc, (u8 *)files);
  SP_CHECK_LAUNCH("sp_png_wrap");
  return SP_OK;
}

extern "C" int sp_png_filter_u8(const void *frames, int n, int h, int w, void *filtered, void *stream) {
  SP_REQUIRE(frames && filtered, "sp_png_filter_u8: null pointer");
  SP_REQUIRE(n > 0 && png_dims_ok(h, w), "sp_png_filter_u8: n must be positive, h and w in 1..65535 and h*w <= 2^24 (n=%d, %dx%d)", n,
             h, w);
  const int64_t grid = (int64_t)n * h;
  SP_REQUIRE(grid <= 0x7fffffff, "sp_png_filter_u8: too many rows (%lld)", (long long)grid);
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const u8 *)frames, h, w,
                     (u8 *)filtered);
  SP_CHECK_LAUNCH("sp_png_filter_u8");
  return SP_OK;
}

extern "C" int sp_png_deflate(const void *filtered, int n, int h, int w, int strip_rows, void *out, size_t cap, void *out_len, void *ws,
                              size_t ws_bytes, void *stream) {
  SP_REQUIRE(filtered && out && out_len && ws, "sp_png_deflate: null pointer");
  SP_REQUIRE(n > 0 && png_dims_ok(h, w), "sp_png_deflate: n must be positive, h and w in 1..65535 and h*w <= 2^24 (n=%d, %dx%d)", n, h,
             w);
  SP_REQUIRE(strip_rows >= 1, "sp_png_deflate: strip_rows %d is not positive", strip_rows);
  PngLayout L;
  png_layout(n, h, w, strip_rows, L);
  const size_t need = sp_png_stream_bytes(h, w, strip_rows);
  SP_REQUIRE(cap >= need, "sp_png_deflate: cap is %zu bytes per frame, a frame can need %zu (sp_png_stream_bytes)", cap, need);
  SP_REQUIRE(ws_bytes >= L.total, "sp_png_deflate: ws holds %zu bytes, needs %zu (sp_png_ws_bytes)", ws_bytes, L.total);
  SP_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)out_len % 4 == 0, "sp_png_deflate: ws must be 8-byte and out_len 4-byte aligned");
  const int64_t grid = (int64_t)n * L.strips;
  SP_REQUIRE(grid <= 0x7fffffff, "sp_png_deflate: too many strips (%lld)", (long long)grid);
  hipStream_t s = (hipStream_t)stream;
  u8 *base = (u8 *)ws;
  int *bits = (int *)(base + L.ints), *offs = bits + grid, *data_bytes = offs + grid;
  u32 *adler = (u32 *)(data_bytes + n);
  u8 *stage = base + L.stage;
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const u8 *)filtered, h, L.pitch, L.rows, L.strips, stage,
                     L.slot, bits, adler);
  hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, (const int *)bits, (const u32 *)adler, h, L.pitch, L.rows,
                     L.strips, offs, data_bytes, (u8 *)out, (int64_t)cap, (int *)out_len);
  hipLaunchKernelGGL(png_place_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const u8 *)stage, L.slot, (const int *)bits,
                     (const int *)offs, L.strips, (u8 *)out, (int64_t)cap);
  SP_CHECK_LAUNCH("sp_png_deflate");
  return SP_OK;
}
