// Baseline JPEG (8-bit, YCbCr 4:2:0, 16x16 MCUs in the order Y00 Y01 Y10 Y11 Cb Cr, Annex K Huffman tables, libjpeg quality
// scaling of the Annex K quantisation tables, restart intervals) of uint8 frames that are already in device memory: what
// the reference's demo leaves to imageio / ffmpeg (/root/reference/scripts/generate_video_demo.py:198-222 save_video /
// save_gif).  The library writes coefficients and entropy-coded scan data; headers and containers are host work.
//
//   jpeg_dct_quant_kernel : one workgroup of 256 per strip of four MCUs (16 rows x 64 pixels).  A thread converts four
//                           pixels of one row (libjpeg's 16-bit fixed-point YCbCr), the 2x2 chroma box sum crosses rows with
//                           one __shfl_xor (rows 2k, 2k+1 sit 16 lanes apart in one wave); the level-shifted planes live in
//                           LDS as fp32, 192 threads run the 8-point row pass and then the column pass of the 24 blocks in
//                           place (separable orthonormal DCT-II, matrix form), then all threads divide, round half away
//                           from zero, clamp the AC terms to +-1023 and store int16 in zigzag order (the strip's 1536
//                           coefficients are contiguous: 512-byte stores per wave).
//   jpeg_entropy_kernel   : one wave per restart interval, 64 blocks at a time, a lane per block.  The tile of coefficients
//                           is staged in LDS (33-word block pitch: a lane per bank); pass 1 counts each block's bits, a wave
//                           prefix sum gives its bit offset, pass 2 ORs its codes into the tile's bit string in LDS (LDS
//                           atomic OR on 32-bit words: neighbours share a word).  Whole bytes then go out 64 at a time, a
//                           ballot over `== 0xFF` giving the stuffed positions; the odd bits are carried into the next
//                           tile.  The DC predictor of a block is the DC of the previous block of its component, read from
//                           the coefficient array itself, so no state runs from block to block.  Each interval goes to a
//                           staging slot of its worst-case size in `ws`.
//   jpeg_scan_kernel      : per frame, the exclusive sum of (interval length + 2 marker bytes) -> offsets, and out_len.
//   jpeg_place_kernel     : one workgroup per interval copies it to its place in the frame's slot and appends RSTm.
// Nothing here is tuned beyond its layout; profiles/jpeg_timing.txt has what it costs.
#include "codec_common.h"

namespace {

// ITU-T T.81 Annex K.1 (natural order)
#define JPEG_LUMA_BASE                                                                                                       \
  {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,                 \
   14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,                 \
   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99}
#define JPEG_CHROMA_BASE                                                                                                     \
  {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, \
   99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}
#define JPEG_ZIGZAG                                                                                                          \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

const u8 h_base[2][64] = {JPEG_LUMA_BASE, JPEG_CHROMA_BASE};
__constant__ u8 d_base[2][64] = {JPEG_LUMA_BASE, JPEG_CHROMA_BASE};
__constant__ u8 d_zigzag[64] = JPEG_ZIGZAG;   // position k of the zigzag sequence -> natural (row-major) position

// libjpeg's jpeg_set_quality + jpeg_add_quant_table (baseline): the one definition host and kernel share
__host__ __device__ inline int quant_entry(int base, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int t = (base * s + 50) / 100;
  return t < 1 ? 1 : (t > 255 ? 255 : t);
}

// ---------------------------------------------------------------------------------------------- DCT + quantisation
struct DctMat { float c[8][8]; };
// c[u][x] = a(u) cos((2x+1) u pi / 16), a(0) = sqrt(1/8), a(u) = 1/2: the angle folded onto [0, pi/2]
constexpr DctMat make_dct() {
  constexpr float half_cos[9] = {0.5f,         0.49039264020161522f, 0.46193976625564337f, 0.41573480615127262f, 0.35355339059327379f,
                                 0.27778511650980114f, 0.19134171618254492f, 0.09754516100806417f, 0.0f};
  DctMat m{};
  for (int u = 0; u < 8; ++u)
    for (int x = 0; x < 8; ++x) {
      int a = ((2 * x + 1) * u) & 31;
      if (a > 16) a = 32 - a;
      float sign = 1.0f;
      if (a > 8) { a = 16 - a; sign = -1.0f; }
      m.c[u][x] = u == 0 ? 0.35355339059327379f : sign * half_cos[a];
    }
  return m;
}

__device__ __forceinline__ void dct8(float (&v)[8]) {
  constexpr DctMat M = make_dct();
  float o[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    float s = 0.0f;
#pragma unroll
    for (int x = 0; x < 8; ++x) s = fmaf(M.c[u][x], v[x], s);
    o[u] = s;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u] = o[u];
}

constexpr int STRIP_MCUS = 4;

__global__ __launch_bounds__(256) void jpeg_dct_quant_kernel(const u8 *__restrict__ frames, int h, int w, int mcu_rows,
                                                             int mcu_cols, int strips, int quality,
                                                             int16_t *__restrict__ coef) {
  __shared__ float yp[16][64];
  __shared__ float cp[2][8][32];
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int strip = (int)(bid % strips);
  const int64_t fr = bid / strips;
  const int my = (int)(fr % mcu_rows);
  const int64_t f = fr / mcu_rows;
  const int mx0 = strip * STRIP_MCUS;

  {  // four pixels of one row per thread; sample (y, x) reads pixel (min(y, h-1), min(x, w-1))
    const int row = tid >> 4, g = tid & 15;
    const int y = min(my * 16 + row, h - 1), x0 = mx0 * 16 + g * 4;
    const u8 *line = frames + (f * h + y) * (int64_t)w * 3;
    u8 px[12];
    const u8 *p = line + (int64_t)x0 * 3;
    if (x0 + 3 < w && ((uintptr_t)p & 3) == 0) {
      const u32 *q = (const u32 *)p;
      const u32 a = q[0], b = q[1], c = q[2];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        px[e] = (u8)(a >> (8 * e));
        px[4 + e] = (u8)(b >> (8 * e));
        px[8 + e] = (u8)(c >> (8 * e));
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const u8 *s = line + (int64_t)min(x0 + e, w - 1) * 3;
        px[3 * e] = s[0]; px[3 * e + 1] = s[1]; px[3 * e + 2] = s[2];
      }
    }
    int cb[4], cr[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = px[3 * e], gg = px[3 * e + 1], b = px[3 * e + 2];
      yp[row][g * 4 + e] = (float)(((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16) - 128);
      cb[e] = (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
      cr[e] = (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
    }
    // h2v2 box: the other row of the pair is 16 lanes away; bias 1 in even output columns, 2 in odd ones
    int s0 = cb[0] + cb[1], s1 = cb[2] + cb[3], t0 = cr[0] + cr[1], t1 = cr[2] + cr[3];
    s0 += __shfl_xor(s0, 16, 64); s1 += __shfl_xor(s1, 16, 64);
    t0 += __shfl_xor(t0, 16, 64); t1 += __shfl_xor(t1, 16, 64);
    if ((row & 1) == 0) {
      cp[0][row >> 1][g * 2] = (float)(((s0 + 1) >> 2) - 128);
      cp[0][row >> 1][g * 2 + 1] = (float)(((s1 + 2) >> 2) - 128);
      cp[1][row >> 1][g * 2] = (float)(((t0 + 1) >> 2) - 128);
      cp[1][row >> 1][g * 2 + 1] = (float)(((t1 + 2) >> 2) - 128);
    }
  }
  __syncthreads();
  // row pass: 16 rows x 8 segments of Y, 2 x 8 rows x 4 segments of chroma; consecutive lanes read consecutive 32 bytes
  if (tid < 192) {
    float *seg = tid < 128 ? &yp[tid >> 3][(tid & 7) * 8] : &cp[(tid - 128) >> 5][((tid - 128) >> 2) & 7][((tid - 128) & 3) * 8];
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = seg[i];
    dct8(v);
#pragma unroll
    for (int i = 0; i < 8; ++i) seg[i] = v[i];
  }
  __syncthreads();
  // column pass: consecutive lanes walk consecutive columns
  if (tid < 192) {
    float *col = tid < 128 ? &yp[(tid >> 6) * 8][tid & 63] : &cp[(tid - 128) >> 5][0][(tid - 128) & 31];
    const int pitch = tid < 128 ? 64 : 32;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = col[i * pitch];
    dct8(v);
#pragma unroll
    for (int i = 0; i < 8; ++i) col[i * pitch] = v[i];
  }
  __syncthreads();
  // 4 MCUs x 6 blocks x 64 = 1536 contiguous int16; 256 and 384 are multiples of 64, so a thread's zigzag index is fixed
  const int k = tid & 63, nat = d_zigzag[k], r = nat >> 3, c = nat & 7;
  const float ql = (float)quant_entry(d_base[0][nat], quality), qc = (float)quant_entry(d_base[1][nat], quality);
  const int valid = min(STRIP_MCUS, mcu_cols - mx0);
  int16_t *dst = coef + ((f * mcu_rows + my) * mcu_cols + mx0) * 384;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int o = j * 256 + tid, m = o / 384, blk = (o - m * 384) >> 6;
    if (m >= valid) continue;
    const float v = blk < 4 ? yp[(blk >> 1) * 8 + r][m * 16 + (blk & 1) * 8 + c] / ql : cp[blk - 4][r][m * 8 + c] / qc;
    int q = (int)roundf(v);                                 // half away from zero
    if (k != 0) q = max(-1023, min(1023, q));               // what baseline Huffman can code (the DC stays within +-1024)
    dst[o] = (int16_t)q;
  }
}

// ---------------------------------------------------------------------------------------------- Huffman tables
// ITU-T T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL; 0 = DC luminance, 1 = DC chrominance, 2 = AC luminance,
// 3 = AC chrominance
struct HuffSpec { u8 bits[16]; int n; u8 vals[162]; };
constexpr HuffSpec SPECS[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
      0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
      0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
      0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
      0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
      0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
      0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
      0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
};

// symbol -> (code << 8) | length, the canonical codes of Annex C; 0 where the table has no code
struct HuffCodes { u32 e[4][256]; };
constexpr HuffCodes make_codes() {
  HuffCodes t{};
  for (int s = 0; s < 4; ++s) {
    u32 code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < SPECS[s].bits[len - 1]; ++i) t.e[s][SPECS[s].vals[k++]] = (code++ << 8) | (u32)len;
      code <<= 1;
    }
  }
  return t;
}
__constant__ HuffCodes d_codes = make_codes();

// ---------------------------------------------------------------------------------------------- entropy coding
constexpr int TILE = 64;                         // blocks per pass: a lane each
constexpr int BLOCK_PITCH = 33;                  // 32-bit words per staged block: lane l starts on bank l (mod 32)
// luminance: DC 9-bit code + 11 bits, AC 16-bit code + 10 bits, 63 times; chrominance stays below (DC 11 + 11, AC <= 12 + 10)
constexpr int BLOCK_BITS = 20 + 63 * 26;
constexpr int BLOCK_BYTES = 2 * ((BLOCK_BITS + 7) / 8);   // 416: every byte may be 0xFF and draw a stuffed zero
constexpr int TILE_WORDS = (7 + TILE * BLOCK_BITS + 31) / 32 + 1;

// Emits (EMIT) or only counts one block's bits.  `cs`: the block's 64 coefficients in zigzag order (LDS); `pred`: the DC
// it is coded against.  Magnitude categories are capped at 15, so int16 values outside the baseline range (AC beyond
// +-1023, DC differences beyond +-2047) give an undecodable stream but never more than BLOCK_BITS bits.
template <bool EMIT>
__device__ __forceinline__ int code_block(const int16_t *cs, int pred, const u32 *dc_tab, const u32 *ac_tab, u32 *bits,
                                          int bit_off) {
  int w = bit_off >> 5, nacc = bit_off & 31, total = 0;
  unsigned long long acc = 0;
  auto put = [&](u32 code, int len) {
    total += len;
    if (EMIT) {
      acc = (acc << len) | code;
      nacc += len;
      if (nacc >= 32) {
        nacc -= 32;
        atomicOr(&bits[w++], (u32)(acc >> nacc));
        acc &= (1ull << nacc) - 1;
      }
    }
  };
  auto value = [&](const u32 *tab, int run, int v) {
    const int a = v < 0 ? -v : v;
    const int size = a ? min(32 - __builtin_clz((u32)a), 15) : 0;
    const u32 e = tab[(run << 4) | size];
    put(e >> 8, (int)(e & 255));
    put((u32)(v < 0 ? v - 1 : v) & ((1u << size) - 1), size);
  };
  value(dc_tab, 0, (int)cs[0] - pred);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = cs[k];
    if (v == 0) { ++run; continue; }
    while (run >= 16) { put(ac_tab[0xF0] >> 8, (int)(ac_tab[0xF0] & 255)); run -= 16; }
    value(ac_tab, run, v);
    run = 0;
  }
  if (run > 0) put(ac_tab[0] >> 8, (int)(ac_tab[0] & 255));
  if (EMIT && nacc > 0) atomicOr(&bits[w], (u32)(acc << (32 - nacc)));
  return total;
}

__device__ __forceinline__ u32 stream_byte(const u32 *bits, int j) { return (bits[j >> 2] >> (24 - 8 * (j & 3))) & 255u; }

// grid: one 64-thread workgroup per (frame, interval).  stage: n_int slots of slot_bytes per frame; lens[frame][interval].
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t *__restrict__ coef, int mcus, int restart_mcus,
                                                          int n_int, u8 *__restrict__ stage, int64_t slot_bytes,
                                                          int *__restrict__ lens) {
  __shared__ u32 tabs[4][256];
  __shared__ u32 cs[TILE * BLOCK_PITCH];
  __shared__ u32 bits[TILE_WORDS];
  const int lane = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int interval = (int)(bid % n_int);
  const int64_t f = bid / n_int;
  const int mcu0 = interval * restart_mcus, m = min(restart_mcus, mcus - mcu0), nblk = 6 * m;
  const int16_t *src = coef + (f * mcus + mcu0) * 384;
  u8 *dst = stage + bid * slot_bytes;
  for (int i = lane; i < 4 * 256; i += 64) (&tabs[0][0])[i] = (&d_codes.e[0][0])[i];

  int carry_bits = 0, out_pos = 0;
  u32 carry_byte = 0;
  for (int b0 = 0; b0 < nblk; b0 += TILE) {
    const int nb = min(TILE, nblk - b0);
    __syncthreads();                                       // the previous tile's bits and coefficients are done with
    {
      const u32 *g = (const u32 *)(src + (int64_t)b0 * 64);
      for (int i = lane; i < nb * 32; i += 64) cs[(i >> 5) * BLOCK_PITCH + (i & 31)] = g[i];
    }
    __syncthreads();
    const int b = b0 + lane, comp = b % 6, mi = b / 6;
    const bool live = lane < nb;
    int pred = 0;
    const int back = comp >= 4 ? 6 : (comp > 0 ? 1 : 3);      // distance to the previous block of the same component
    if (live && ((comp > 0 && comp < 4) || mi > 0)) pred = src[(int64_t)(b - back) * 64];
    const int16_t *mine = (const int16_t *)&cs[lane * BLOCK_PITCH];
    const u32 *dc_tab = tabs[comp >= 4 ? 1 : 0], *ac_tab = tabs[comp >= 4 ? 3 : 2];
    const int nbits = live ? code_block<false>(mine, pred, dc_tab, ac_tab, nullptr, 0) : 0;
    const int incl = wave_inclusive_sum(nbits);
    int total = carry_bits + __shfl(incl, 63, 64);
    for (int i = lane; i <= (total >> 5); i += 64) bits[i] = i == 0 ? carry_byte << 24 : 0u;
    __syncthreads();
    if (live) code_block<true>(mine, pred, dc_tab, ac_tab, bits, carry_bits + incl - nbits);
    const bool last = b0 + TILE >= nblk;
    if (last && (total & 7)) {                             // pad the interval to a byte with 1-bits
      const int pad = 8 - (total & 7);
      if (lane == 0) atomicOr(&bits[total >> 5], ((1u << pad) - 1) << (32 - (total & 31) - pad));
      total += pad;
    }
    __syncthreads();
    const int nbytes = total >> 3;
    for (int j0 = 0; j0 < nbytes; j0 += 64) {
      const int j = j0 + lane;
      const u32 v = j < nbytes ? stream_byte(bits, j) : 0u;
      const unsigned long long ff = __ballot(v == 255u);
      const int at = out_pos + lane + __popcll(ff & ((1ull << lane) - 1));
      if (j < nbytes) {
        dst[at] = (u8)v;
        if (v == 255u) dst[at + 1] = 0;
      }
      out_pos += min(64, nbytes - j0) + __popcll(ff);
    }
    carry_bits = total & 7;
    carry_byte = carry_bits ? stream_byte(bits, nbytes) : 0u;
  }
  if (lane == 0) lens[bid] = out_pos;
}

// offs[f][k] = sum_{j<k} (lens[f][j] + 2); out_len[f] = the whole segment (no marker after the last interval)
__global__ __launch_bounds__(256) void jpeg_scan_kernel(const int *__restrict__ lens, int n_int, int *__restrict__ offs,
                                                        int *__restrict__ out_len) {
  __shared__ int wave_tot[4];
  const int64_t f = blockIdx.x;
  const int running = carried_exclusive_sum(
      wave_tot, n_int, 0, [&](int k) { return lens[f * n_int + k] + 2; }, [&](int k, int before) { offs[f * n_int + k] = before; });
  if (threadIdx.x == 0) out_len[f] = running - 2;
}

__global__ __launch_bounds__(256) void jpeg_place_kernel(const u8 *__restrict__ stage, int64_t slot_bytes,
                                                         const int *__restrict__ lens, const int *__restrict__ offs, int n_int,
                                                         u8 *__restrict__ out, int64_t cap) {
  const int64_t bid = blockIdx.x;
  const int interval = (int)(bid % n_int);
  const int64_t f = bid / n_int;
  const int len = lens[bid];
  const u8 *src = stage + bid * slot_bytes;
  u8 *dst = out + f * cap + offs[bid];
  for (int i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
  if (threadIdx.x == 0 && interval + 1 < n_int) {
    dst[len] = 0xFF;
    dst[len + 1] = (u8)(0xD0 + (interval & 7));
  }
}

bool jpeg_dims_ok(int h, int w) { return h > 0 && w > 0 && h <= 65535 && w <= 65535; }
int64_t jpeg_intervals(int64_t mcus, int restart_mcus) { return (mcus + restart_mcus - 1) / restart_mcus; }

}  // namespace

extern "C" int sp_jpeg_quant_tables(int quality, uint8_t *luma64, uint8_t *chroma64) {
  SP_REQUIRE(luma64 && chroma64, "sp_jpeg_quant_tables: null pointer");
  SP_REQUIRE(quality >= 1 && quality <= 100, "sp_jpeg_quant_tables: quality %d is not in 1..100", quality);
  for (int i = 0; i < 64; ++i) {
    luma64[i] = (uint8_t)quant_entry(h_base[0][i], quality);
    chroma64[i] = (uint8_t)quant_entry(h_base[1][i], quality);
  }
  return SP_OK;
}

extern "C" int sp_jpeg_huffman_table(int which, uint8_t *bits16, uint8_t *vals162) {
  SP_REQUIRE(bits16 && vals162, "sp_jpeg_huffman_table: null pointer");
  SP_REQUIRE(which >= 0 && which < 4, "sp_jpeg_huffman_table: table %d is not one of 0..3", which);
  for (int i = 0; i < 16; ++i) bits16[i] = SPECS[which].bits[i];
  for (int i = 0; i < SPECS[which].n; ++i) vals162[i] = SPECS[which].vals[i];
  return SPECS[which].n;
}

extern "C" size_t sp_jpeg_coef_bytes(int n, int h, int w) {
  if (n <= 0 || !jpeg_dims_ok(h, w)) return 0;
  return (size_t)n * (size_t)((h + 15) / 16) * (size_t)((w + 15) / 16) * 6 * 64 * sizeof(int16_t);
}

extern "C" int sp_jpeg_dct_quant_u8(const void *frames, int n, int h, int w, int quality, void *coef, void *stream) {
  SP_REQUIRE(frames && coef, "sp_jpeg_dct_quant_u8: null pointer");
  SP_REQUIRE(n > 0 && jpeg_dims_ok(h, w), "sp_jpeg_dct_quant_u8: n must be positive, h and w in 1..65535 (n=%d, %dx%d)", n, h, w);
  SP_REQUIRE(quality >= 1 && quality <= 100, "sp_jpeg_dct_quant_u8: quality %d is not in 1..100", quality);
  SP_REQUIRE((uintptr_t)coef % 2 == 0, "sp_jpeg_dct_quant_u8: coef must be 2-byte aligned");
  const int mcu_rows = (h + 15) / 16, mcu_cols = (w + 15) / 16, strips = (mcu_cols + STRIP_MCUS - 1) / STRIP_MCUS;
  const int64_t blocks = (int64_t)n * mcu_rows * strips;
  SP_REQUIRE(blocks <= 0x7fffffff, "sp_jpeg_dct_quant_u8: too many MCU strips (%lld)", (long long)blocks);
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(jpeg_dct_quant_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const u8 *)frames, h, w,
                     mcu_rows, mcu_cols, strips, quality, (int16_t *)coef);
  SP_CHECK_LAUNCH("sp_jpeg_dct_quant_u8");
  return SP_OK;
}

extern "C" size_t sp_jpeg_stream_bytes(int h, int w, int restart_mcus) {
  if (!jpeg_dims_ok(h, w) || restart_mcus < 1 || restart_mcus > 65535) return 0;
  const int64_t mcus = (int64_t)((h + 15) / 16) * ((w + 15) / 16);
  return (size_t)mcus * 6 * BLOCK_BYTES + 2 * (size_t)(jpeg_intervals(mcus, restart_mcus) - 1);
}

extern "C" size_t sp_jpeg_entropy_ws_bytes(int n, int mcu_rows, int mcu_cols, int restart_mcus) {
  if (n <= 0 || mcu_rows <= 0 || mcu_cols <= 0 || mcu_rows > 4096 || mcu_cols > 4096 || restart_mcus < 1 || restart_mcus > 65535)
    return 0;
  const int64_t mcus = (int64_t)mcu_rows * mcu_cols, n_int = jpeg_intervals(mcus, restart_mcus);
  const size_t slot = (size_t)(mcus < restart_mcus ? mcus : restart_mcus) * 6 * BLOCK_BYTES;
  return align256(2 * sizeof(int) * (size_t)n * (size_t)n_int) + (size_t)n * (size_t)n_int * slot;
}

extern "C" int sp_jpeg_entropy(const void *coef, int n, int mcu_rows, int mcu_cols, int restart_mcus, void *out, size_t cap,
                               void *out_len, void *ws, size_t ws_bytes, void *stream) {
  SP_REQUIRE(coef && out && out_len && ws, "sp_jpeg_entropy: null pointer");
  SP_REQUIRE(n > 0 && mcu_rows > 0 && mcu_cols > 0 && mcu_rows <= 4096 && mcu_cols <= 4096,
             "sp_jpeg_entropy: n must be positive, mcu_rows and mcu_cols in 1..4096 (n=%d, %dx%d)", n, mcu_rows, mcu_cols);
  SP_REQUIRE(restart_mcus >= 1 && restart_mcus <= 65535, "sp_jpeg_entropy: restart_mcus %d is not in 1..65535", restart_mcus);
  const int64_t mcus = (int64_t)mcu_rows * mcu_cols, n_int = jpeg_intervals(mcus, restart_mcus);
  const size_t need = (size_t)mcus * 6 * BLOCK_BYTES + 2 * (size_t)(n_int - 1);
  SP_REQUIRE(need <= 0x7fffffff, "sp_jpeg_entropy: a frame of %lld MCUs can pass 2^31 bytes (out_len is int32)", (long long)mcus);
  SP_REQUIRE(cap >= need, "sp_jpeg_entropy: cap is %zu bytes per frame, a frame can need %zu (sp_jpeg_stream_bytes)", cap, need);
  SP_REQUIRE(ws_bytes >= sp_jpeg_entropy_ws_bytes(n, mcu_rows, mcu_cols, restart_mcus),
             "sp_jpeg_entropy: ws holds %zu bytes, needs %zu", ws_bytes, sp_jpeg_entropy_ws_bytes(n, mcu_rows, mcu_cols, restart_mcus));
  SP_REQUIRE((uintptr_t)coef % 4 == 0 && (uintptr_t)ws % 4 == 0 && (uintptr_t)out_len % 4 == 0,
             "sp_jpeg_entropy: coef, ws and out_len must be 4-byte aligned");
  SP_REQUIRE((int64_t)n * n_int <= 0x7fffffff, "sp_jpeg_entropy: too many restart intervals (%lld)", (long long)((int64_t)n * n_int));
  hipStream_t s = (hipStream_t)stream;
  int *lens = (int *)ws, *offs = lens + (int64_t)n * n_int;
  u8 *stage = (u8 *)ws + align256(2 * sizeof(int) * (size_t)n * (size_t)n_int);
  const int64_t slot = (mcus < restart_mcus ? mcus : restart_mcus) * 6 * BLOCK_BYTES;
  const dim3 per_interval((unsigned)((int64_t)n * n_int));
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(jpeg_entropy_kernel, per_interval, dim3(64), 0, s, (const int16_t *)coef, (int)mcus, restart_mcus, (int)n_int,
                     stage, slot, lens);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, (const int *)lens, (int)n_int, offs, (int *)out_len);
  hipLaunchKernelGGL(jpeg_place_kernel, per_interval, dim3(256), 0, s, (const u8 *)stage, slot, (const int *)lens, (const int *)offs,
                     (int)n_int, (u8 *)out, (int64_t)cap);
  SP_CHECK_LAUNCH("sp_jpeg_entropy");
  return SP_OK;
}
