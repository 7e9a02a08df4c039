// fp8 (OCP e4m3fn) feed-forward path: LayerNorm + per-row quantisation, and a row-/column-scaled W8A8 contraction on the
// block-scaled MFMA v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (the one fp8 form at twice the fp16 rate).
//
//   sp_ln_quant_f8 : q[m][:] = e4m3((x[m][:] - mean[m]) * rstd[m] / sa[m]),  sa[m] = max|y| / 448
//   sp_gemm_f8     : D[m][:] = epilogue(sa[m] * sw[n] * sum_k A8[m][k] * W8[n][k] + bias[n])
//
// Contraction: 256 threads, one wave per SIMD; a workgroup owns 256 rows x 256 weight rows (128
// stored columns under GEGLU), a wave 128 x 128 as 4 x 4 accumulator tiles of 32 x 32 (256 registers, unified file).  K
// moves in whole 128-byte lines per row -- two MFMA k-steps -- staged by global_load_lds_dwordx4 into two ping-pong
// stages of (32 + 32) KB.  LDS image of a stage: row r at r*128, the 16-byte piece c of its line at position
// c ^ swz(r), swz(r) = (r ^ (r >> 3)) & 7: the 16 (or 8) consecutive rows one ds_read_b128 pass covers land on distinct
// banks, for 64 and for 32 banks alike.  Lane l of a fragment holds row l & 31 and, of the 64 k bytes of a k-step, pieces
// 2h and 2h + 1 (h = l >> 5): one ds_read_b128 each, the same assignment for A and W, which is all the instruction needs
// (it sums over k; tools/fp8_scale_probe.hip).  The weight fragment is the MFMA's first operand: a lane then owns ONE
// output row and, per accumulator tile, weight rows 8g + 4h .. + 3 (g = 0..3) -- with the GEGLU interleave in blocks of
// 16, value (g = 0, 1) and gate (g = 2, 3) of the same output column sit in the same lane.
#include "gemm_args.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int F8_BM = 256, F8_BN = 256, F8_LINE = 128;
constexpr int F8_A_BYTES = F8_BM * F8_LINE;                 // 32 KB
constexpr int F8_STAGE = (F8_BM + F8_BN) * F8_LINE;         // 64 KB
constexpr int F8_LDS = 2 * F8_STAGE;                        // 128 KB; the epilogue's 256 x 256 fp16 tile is as large

struct F8Args {
  const uint8_t *a, *w;
  const float *sa, *sw, *bias;
  const f16 *res1;
  f16 *d;
  int64_t lda, ldr1, ldd;
  float r1scale;
  int m, n, k, tiles_m, tiles_n;
};

template <bool GEGLU>
__global__ __launch_bounds__(256) void gemm_f8_kernel(const F8Args p) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // column tiles of one row tile run back to back on one XCD: the A rows are fetched from HBM once
  const int t = spgemm::xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = t / p.tiles_n, tile_n = t - tile_m * p.tiles_n;
  const int64_t mbase = (int64_t)tile_m * F8_BM;

  // ---- LDS-DMA: piece pc = i*4 + wave of an operand is its rows 8*pc .. 8*pc + 7, one whole line per 8 lanes.  The lane
  // that lands at position lpos of row r fetches source piece lpos ^ swz(r); swz(r) = lrow ^ (pc & 7) depends on i only
  // through its parity.  Rows at or beyond m (n) are read from row m - 1 (n - 1) and never stored.
  const int lrow = lane >> 3, lpos = lane & 7;
  const int c0 = lpos ^ lrow ^ wave;                        // source piece for even i; odd i: c0 ^ 4
  const uint8_t *arow[8], *wrow[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = (i * 4 + wave) * 8 + lrow;
    const int64_t am = min(mbase + r, (int64_t)p.m - 1);
    const int wr = min(tile_n * F8_BN + r, p.n - 1);
    arow[i] = p.a + am * p.lda;
    wrow[i] = p.w + (int64_t)wr * p.k;
  }
  // K = 128*j + 64: the last stage is half a line.  Its lanes of pieces 4..7 fetch pieces 0..3 again (inside the row), and
  // the second k-step of that stage is not multiplied.
  auto stage = [&](int kt) {
    char *sa_ = smem + (kt & 1) * F8_STAGE;
    char *sb_ = sa_ + F8_A_BYTES;
    const bool half = p.k - kt * F8_LINE < F8_LINE;
    const int o0 = kt * F8_LINE + ((half ? (c0 & 3) : c0) << 4);
    const int o1 = kt * F8_LINE + ((half ? (c0 & 3) : (c0 ^ 4)) << 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) glds16(arow[i] + ((i & 1) ? o1 : o0), sa_ + (i * 4 + wave) * 1024);
#pragma unroll
    for (int i = 0; i < 8; ++i) glds16(wrow[i] + ((i & 1) ? o1 : o0), sb_ + (i * 4 + wave) * 1024);
  };

  f32x16 acc[4][4];                                         // [weight tile][row tile]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int lr = lane & 31, h = lane >> 5;
  const int nk2 = (p.k + F8_LINE - 1) / F8_LINE;
  // the last column tile may be half a tile: its right-hand waves stage their share and multiply nothing
  const bool active = tile_n * F8_BN + wn * 128 < p.n;
  const int a_off = (wm * 128 + lr) * F8_LINE, w_off = (wn * 128 + lr) * F8_LINE;
  // swz of fragment row 32*T + lr: (lr & 7) ^ (4*(T & 1) + (lr >> 3)); T & 1 is the tile index' parity (wave bases are 128)
  const int sz0 = ((lr & 7) ^ (lr >> 3)) & 7, sz1 = sz0 ^ 4;

  stage(0);
  for (int kt = 0; kt < nk2; ++kt) {
    // stage kt has landed (this wave's share; the barrier makes it everyone's), and every wave is done reading the other
    // stage, which the next DMA overwrites
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (kt + 1 < nk2) stage(kt + 1);
    if (active) {
      const char *sa_ = smem + (kt & 1) * F8_STAGE;
      const char *sb_ = sa_ + F8_A_BYTES;
      const int steps = p.k - kt * F8_LINE >= F8_LINE ? 2 : 1;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s < steps) {
          i32x8 fa[4], fw[4];
          const int c = 4 * s + 2 * h;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int sz = (u & 1) ? sz1 : sz0;
            const int p0 = (c ^ sz) << 4, p1 = ((c + 1) ^ sz) << 4;
            const i32x4 al = *(const i32x4 *)(sa_ + a_off + u * (32 * F8_LINE) + p0);
            const i32x4 ah = *(const i32x4 *)(sa_ + a_off + u * (32 * F8_LINE) + p1);
            const i32x4 wl = *(const i32x4 *)(sb_ + w_off + u * (32 * F8_LINE) + p0);
            const i32x4 wh = *(const i32x4 *)(sb_ + w_off + u * (32 * F8_LINE) + p1);
            fa[u] = (i32x8){al[0], al[1], al[2], al[3], ah[0], ah[1], ah[2], ah[3]};
            fw[u] = (i32x8){wl[0], wl[1], wl[2], wl[3], wh[0], wh[1], wh[2], wh[3]};
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)       // e4m3 x e4m3 (cbsz = blgp = 0), both block scales E8M0 127 = 1.0
              acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[i], fa[j], acc[i][j], 0, 0, 0, 127, 0, 127);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");     // the stages are free: the tile goes there

  // ---- epilogue.  acc[i][j][4g + r]: weight row tile_n*256 + wn*128 + 32i + 8g + 4h + r, output row mbase + wm*128 + 32j + lr.
  // Scale and bias in fp32, GEGLU or the residual in fp32, ONE rounding to fp16; the tile is staged in LDS (rows of bno
  // halves, 16-byte piece c of row r at c ^ (r & 15)) and leaves as 16-byte coalesced stores.
  constexpr int bno = GEGLU ? F8_BN / 2 : F8_BN;
  constexpr int cpr = bno / 8;
  const int ncols = GEGLU ? p.n / 2 : p.n;
  if (active) {
    float sar[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sar[j] = p.sa[min(mbase + wm * 128 + 32 * j + lr, (int64_t)p.m - 1)];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n0 = tile_n * F8_BN + wn * 128 + 32 * i + 4 * h;
      f32x4 swv[4], bv[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        swv[g] = *(const f32x4 *)(p.sw + n0 + 8 * g);
        bv[g] = *(const f32x4 *)(p.bias + n0 + 8 * g);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rl = wm * 128 + 32 * j + lr;
        char *srow = smem + rl * (bno * 2);
        if constexpr (GEGLU) {
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            f16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float hv = fmaf(sar[j] * swv[g][r], acc[i][j][4 * g + r], bv[g][r]);
              const float gv = fmaf(sar[j] * swv[g + 2][r], acc[i][j][4 * (g + 2) + r], bv[g + 2][r]);
              o[r] = (f16)(hv * gelu_f(gv));
            }
            const int col = wn * 64 + 16 * i + 8 * g + 4 * h;
            *(f16x4 *)(srow + (((col >> 3) ^ (rl & 15)) << 4) + (col & 4) * 2) = o;
          }
        } else {
          const int64_t mrow = mbase + rl;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int col = wn * 128 + 32 * i + 8 * g + 4 * h;
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaf(sar[j] * swv[g][r], acc[i][j][4 * g + r], bv[g][r]);
            if (p.res1 && mrow < p.m) {
              const f16x4 q = *(const f16x4 *)(p.res1 + mrow * p.ldr1 + tile_n * F8_BN + col);
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] = fmaf(p.r1scale, (float)q[r], v[r]);
            }
            const f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
            *(f16x4 *)(srow + (((col >> 3) ^ (rl & 15)) << 4) + (col & 4) * 2) = o;
          }
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll 4
  for (int it = 0; it < cpr; ++it) {
    const int idx = tid + it * 256;
    const int r = idx / cpr, c = idx - r * cpr;
    const int64_t mrow = mbase + r;
    const int col = tile_n * bno + c * 8;                   // ncols is a multiple of 64: a piece is stored whole or not at all
    if (mrow < p.m && col < ncols)
      *(f16x8 *)(p.d + mrow * p.ldd + col) = *(const f16x8 *)(smem + r * (bno * 2) + ((c ^ (r & 15)) << 4));
  }
}

// LayerNorm + e4m3 rows.  LPR lanes share a row, a lane owns the 16-channel groups j*LPR + li (two 16-byte loads, one
// 16-byte store each); a wave covers 64 / LPR rows.  No LDS: the row maximum is log2(LPR) shuffle steps.
template <int LPR, int NG>
__global__ __launch_bounds__(256) void ln_quant_f8_kernel(const f16 *__restrict__ x, int64_t ldx, const float *__restrict__ stats,
                                                          uint8_t *__restrict__ q, int64_t ldq, float *__restrict__ sa,
                                                          int64_t rows, int ngroups) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, li = lane % LPR;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
  const int64_t rr = row < rows ? row : rows - 1;           // (clamped rows are computed, not stored)
  const float2 st = *(const float2 *)(stats + rr * 2);
  float y[NG][16];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int g = j * LPR + li;
    if (g < ngroups) {
      const f16x8 v0 = *(const f16x8 *)(x + rr * ldx + g * 16), v1 = *(const f16x8 *)(x + rr * ldx + g * 16 + 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        y[j][e] = ((float)v0[e] - st.x) * st.y;
        y[j][e + 8] = ((float)v1[e] - st.x) * st.y;
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(y[j][e]));
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) y[j][e] = 0.f;
    }
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
  const float inv = amax > 0.f ? 448.0f / amax : 0.0f;
  if (row >= rows) return;
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int g = j * LPR + li;
    if (g < ngroups) {
      i32x4 o;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        float v[4];
#pragma unroll      // the conversion does not saturate by itself: 448*(1 + ulp) must not become the NaN code
        for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(y[j][4 * d + e] * inv, -448.0f, 448.0f);
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w, true);
        o[d] = w;
      }
      *(i32x4 *)(q + row * ldq + g * 16) = o;
    }
  }
  if (li == 0) sa[row] = scale;
}

bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

}  // namespace

extern "C" int sp_ln_quant_f8(const void *x, int64_t ldx, const float *stats, void *q, int64_t ldq, float *sa, int64_t rows,
                              int c, void *stream) {
  SP_REQUIRE(x, "sp_ln_quant_f8: x is null");
  SP_REQUIRE(stats, "sp_ln_quant_f8: stats is null");
  SP_REQUIRE(q, "sp_ln_quant_f8: q is null");
  SP_REQUIRE(sa, "sp_ln_quant_f8: sa is null");
  SP_REQUIRE(rows > 0 && rows < ((int64_t)1 << 31), "sp_ln_quant_f8: rows=%lld must be positive and below 2^31", (long long)rows);
  SP_REQUIRE(c >= 64 && c <= 1280 && c % 64 == 0, "sp_ln_quant_f8: c=%d must be a multiple of 64 in 64 .. 1280", c);
  SP_REQUIRE(ldx >= c && ldx % 8 == 0, "sp_ln_quant_f8: ldx=%lld must be >= c and a multiple of 8", (long long)ldx);
  SP_REQUIRE(ldq >= c && ldq % 16 == 0, "sp_ln_quant_f8: ldq=%lld must be >= c and a multiple of 16", (long long)ldq);
  SP_REQUIRE(aligned16(x), "sp_ln_quant_f8: x must be 16-byte aligned");
  SP_REQUIRE(aligned16(q), "sp_ln_quant_f8: q must be 16-byte aligned");
  SP_REQUIRE(((uintptr_t)stats & 7) == 0, "sp_ln_quant_f8: stats must be 8-byte aligned");
  SP_REQUIRE(((uintptr_t)sa & 3) == 0, "sp_ln_quant_f8: sa must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  SP_CLEAR_STALE_ERROR();
#define LNQ(LPR, NG)                                                                                                       \
  hipLaunchKernelGGL((ln_quant_f8_kernel<LPR, NG>), dim3((unsigned)((rows + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)))),     \
                     dim3(256), 0, s, (const f16 *)x, ldx, stats, (uint8_t *)q, ldq, sa, rows, c / 16)
  // rows per wave as sp_ln_stats_f16 has them for the UNet's widths (its 2 passes of 8 / 4 / 2 rows), one row per wave else
  if (c == 320 && rows >= 8192) LNQ(4, 5);
  else if (c == 640 && rows >= 4096) LNQ(8, 5);
  else if (c == 1280 && rows >= 2048) LNQ(16, 5);
  else LNQ(64, 2);
#undef LNQ
  SP_CHECK_LAUNCH("sp_ln_quant_f8");
  return SP_OK;
}

extern "C" int sp_gemm_f8(const void *a8, int64_t lda, const float *sa, const void *w8, const float *sw, const float *bias,
                          const void *res1, int64_t ldr1, float r1scale, void *d, int64_t ldd, int m, int n, int k, int geglu,
                          void *stream) {
  SP_REQUIRE(a8, "sp_gemm_f8: a8 is null");
  SP_REQUIRE(sa, "sp_gemm_f8: sa is null");
  SP_REQUIRE(w8, "sp_gemm_f8: w8 is null");
  SP_REQUIRE(sw, "sp_gemm_f8: sw is null");
  SP_REQUIRE(bias, "sp_gemm_f8: bias is null");
  SP_REQUIRE(d, "sp_gemm_f8: d is null");
  SP_REQUIRE(m > 0, "sp_gemm_f8: m=%d must be positive", m);
  SP_REQUIRE(n > 0 && n % 128 == 0, "sp_gemm_f8: n=%d must be a positive multiple of 128", n);
  SP_REQUIRE(k >= 64 && k <= 1280 && k % 64 == 0, "sp_gemm_f8: k=%d must be a multiple of 64 in 64 .. 1280", k);
  const int nout = geglu ? n / 2 : n;
  SP_REQUIRE(lda >= k && lda % 16 == 0, "sp_gemm_f8: lda=%lld must be >= k and a multiple of 16", (long long)lda);
  SP_REQUIRE(ldd >= nout && ldd % 8 == 0, "sp_gemm_f8: ldd=%lld must be >= the stored columns and a multiple of 8", (long long)ldd);
  SP_REQUIRE(!(geglu && res1), "sp_gemm_f8: res1 is not part of the geglu epilogue");
  if (res1) SP_REQUIRE(ldr1 >= nout && ldr1 % 8 == 0, "sp_gemm_f8: ldr1=%lld must be >= n and a multiple of 8", (long long)ldr1);
  SP_REQUIRE(aligned16(a8), "sp_gemm_f8: a8 must be 16-byte aligned");
  SP_REQUIRE(aligned16(w8), "sp_gemm_f8: w8 must be 16-byte aligned");
  SP_REQUIRE(aligned16(sw), "sp_gemm_f8: sw must be 16-byte aligned");
  SP_REQUIRE(aligned16(bias), "sp_gemm_f8: bias must be 16-byte aligned");
  SP_REQUIRE(aligned16(d), "sp_gemm_f8: d must be 16-byte aligned");
  SP_REQUIRE(aligned16(res1), "sp_gemm_f8: res1 must be 16-byte aligned");
  SP_REQUIRE(((uintptr_t)sa & 3) == 0, "sp_gemm_f8: sa must be 4-byte aligned");
  F8Args a{};
  a.a = (const uint8_t *)a8; a.w = (const uint8_t *)w8;
  a.sa = sa; a.sw = sw; a.bias = bias;
  a.res1 = (const f16 *)res1; a.d = (f16 *)d;
  a.lda = lda; a.ldr1 = ldr1; a.ldd = ldd; a.r1scale = r1scale;
  a.m = m; a.n = n; a.k = k;
  a.tiles_m = (m + F8_BM - 1) / F8_BM;
  a.tiles_n = (n + F8_BN - 1) / F8_BN;
  SP_REQUIRE((int64_t)a.tiles_m * a.tiles_n < ((int64_t)1 << 31), "sp_gemm_f8: m=%d x n=%d is more tiles than a grid holds", m, n);
  spgemm::note_kernel("gemm_f8_kernel<256, 256, %d>", geglu ? 1 : 0);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(a.tiles_m * a.tiles_n));
  if (geglu) {
    static bool attr_set[SP_MAX_DEVICES] = {};
    if (int rc = sp_ensure_dyn_lds((const void *)gemm_f8_kernel<true>, F8_LDS, attr_set, "sp_gemm_f8")) return rc;
    SP_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(gemm_f8_kernel<true>, grid, dim3(256), F8_LDS, s, a);
  } else {
    static bool attr_set[SP_MAX_DEVICES] = {};
    if (int rc = sp_ensure_dyn_lds((const void *)gemm_f8_kernel<false>, F8_LDS, attr_set, "sp_gemm_f8")) return rc;
    SP_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(gemm_f8_kernel<false>, grid, dim3(256), F8_LDS, s, a);
  }
  SP_CHECK_LAUNCH("sp_gemm_f8");
  return SP_OK;
}
