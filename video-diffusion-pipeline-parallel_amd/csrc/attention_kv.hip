// Spatial self-attention over POOLED keys and values for gfx950 (head_dim 64, fp16 in, fp32 logits and statistics, no
// mask): every query token of a frame attends over K and V averaged over f x f cells of the frame's token grid, so a
// frame of seq_q tokens meets seq_kv = seq_q / f^2 keys.  Two entry points:
//
// sp_kv_pool_f16 -- kv_pool_kernel<F>.  One thread per (pooled row, 16-byte piece of the row): it loads the F*F source
//   pieces of K and of V that fall into its cell (each source piece is loaded by exactly one thread, once), sums them in
//   fp32 in a fixed order, multiplies by 1/F^2 and stores 16 bytes of Kp and of Vp, rounded once.  Consecutive threads
//   take consecutive pieces of one row, so every load and store instruction covers whole rows.  No LDS, memory-bound.
//
// sp_attn_spatial_kv_f16 -- attn_kv_kernel: rectangular flash attention, seq_q queries against seq_kv keys.
//  * Workgroup = 4 waves = 256 consecutive query rows of one (image, head), two workgroups per CU.  Wave w owns TWO
//    32-query blocks (rows 64w .. 64w+31 and 64w+32 .. 64w+63): with the key loop f^2 times shorter than the square
//    kernel's, what is paid once per workgroup (Q fetch, first tile's latency, epilogue) and once per tile (barrier,
//    LDS operand reads) weighs more, and every K and V^T fragment read from LDS here feeds two MFMAs instead of one.
//    Consecutive workgroups are the query blocks of one (image, head): its pooled K and V (295 KB each at 2,304
//    keys) stay in L2 while they run.
//  * K/V stream through LDS in 64-key tiles, 8 KB for K and 8 KB for V, double-buffered (32 KB per workgroup): tile
//    t+1 is in flight (global_load_lds_dwordx4, two 1-KiB pieces of K and of V per wave) while tile t is consumed;
//    one barrier per tile.  Tile bases are loop-carried (one 64-bit add per operand and tile), the lane part of a
//    source address is computed once.  The 16-byte chunk c of tile row `row` sits at chunk c ^ ((row >> 1) & 7) for K
//    (conflict-free ds_read_b128 operand reads) and at c ^ (((row >> 1) & 1) << 2) for V (conflict-free
//    ds_read_b64_tr_b16), both applied on the source side of the DMA, as in attention.hip.
//  * Both products are transposed, S^T = K.Q^T and O^T += V^T.P^T on v_mfma_f32_32x32x16_f16: a lane holds 32 scores of
//    ONE query (the row maximum needs one exchange with the lane 32 away), and the score registers, rounded to fp16 in
//    place, are the B operand of the second product: P never goes through LDS.  V arrives row-major; V^T fragments
//    come out of the row-major tile through the transposing LDS read.
//  * Plain online softmax per tile and query block: fp32 logits straight from the MFMA (Q is NOT pre-scaled), running
//    maximum m and sum l in fp32, p = exp2(s * c - m * c) with c = scale * log2(e) as one fma in front of v_exp_f32;
//    l adds the unrounded fp32 p.  O and l are rescaled only in tiles where some row's maximum rose (wave-uniform).
//  * Tails: a key row at or beyond seq_kv is fetched from row seq_kv - 1 of its image and its logit is set to -inf
//    before the maximum (p is exactly 0); a query row at or beyond seq_q is computed on row seq_q - 1 and not stored.
//    No address leaves rows [b*seq, (b+1)*seq) and columns [64 head, 64 head + 64) of any operand; no zero page.
#include "common.h"

namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int KVA_TILE = 64;     // keys per tile
constexpr int KVA_ROWS = 256;    // query rows per workgroup
constexpr int KVA_QB = 2;        // 32-query blocks per wave

// ------------------------------------------------------------------------------------------------
template <int F>
__global__ __launch_bounds__(256) void kv_pool_kernel(const f16 *__restrict__ k, const f16 *__restrict__ v, int64_t ldk,
                                                      int64_t ldv, f16 *__restrict__ kp, f16 *__restrict__ vp,
                                                      int64_t ldkp, int64_t ldvp, int h, int w, int c8, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int wo = w / F, ho = h / F;
  const int piece = (int)(idx % c8);
  const int64_t orow = idx / c8;
  const int x = (int)(orow % wo), y = (int)((orow / wo) % ho);
  const int64_t img = orow / ((int64_t)wo * ho);
  const int64_t src0 = (img * h + (int64_t)y * F) * w + (int64_t)x * F;     // top-left token of the cell

  f16x8 kr[F * F], vr[F * F];
#pragma unroll
  for (int dy = 0; dy < F; ++dy)
#pragma unroll
    for (int dx = 0; dx < F; ++dx) {
      const int64_t row = src0 + (int64_t)dy * w + dx;
      kr[dy * F + dx] = *(const f16x8 *)(k + row * ldk + piece * 8);
      vr[dy * F + dx] = *(const f16x8 *)(v + row * ldv + piece * 8);
    }
  constexpr float inv = 1.0f / (F * F);
  f16x8 ko, vo;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float sk = 0.f, sv = 0.f;
#pragma unroll
    for (int i = 0; i < F * F; ++i) { sk += (float)kr[i][e]; sv += (float)vr[i][e]; }
    ko[e] = (f16)(sk * inv);          // (one rounding, to nearest even)
    vo[e] = (f16)(sv * inv);
  }
  *(f16x8 *)(kp + orow * ldkp + piece * 8) = ko;
  *(f16x8 *)(vp + orow * ldvp + piece * 8) = vo;
}

// ------------------------------------------------------------------------------------------------
// grid.x = (image, head) major, query block of 256 rows minor
__global__ __launch_bounds__(256, 2) void attn_kv_kernel(
    const f16 *__restrict__ q, const f16 *__restrict__ k, const f16 *__restrict__ v, f16 *__restrict__ o, int64_t ldq,
    int64_t ldk, int64_t ldv, int64_t ldo, int seq_q, int seq_kv, int heads, int nblk, float scale_log2e) {
  constexpr int KV = KVA_TILE, QB = KVA_QB;
  constexpr int K_BYTES = KV * 128, STAGE = 2 * K_BYTES;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.x / nblk, blk = blockIdx.x - bh * nblk;
  const int b = bh / heads, hd = bh - b * heads;
  const int r = lane & 31, h = lane >> 5;
  const int q0 = blk * KVA_ROWS + wave * (32 * QB);

  // Q fragments (B operand of S^T = K.Q^T): lane (r, h) holds Q[q0 + 32 j + r][16 s + 8 h .. + 7]; rows past seq_q
  // repeat row seq_q - 1
  f16x8 qf[QB][4];
  int64_t qrow[QB];
#pragma unroll
  for (int j = 0; j < QB; ++j) {
    qrow[j] = (int64_t)b * seq_q + min(q0 + 32 * j + r, seq_q - 1);
    const f16 *qp = q + qrow[j] * ldq + hd * 64 + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[j][s] = *(const f16x8 *)(qp + 16 * s);
  }

  // K/V staging: each wave moves 16 rows of K and of V per tile (2 + 2 LDS-DMA pieces of 8 rows x 128 bytes).  Source
  // address = loop-carried base of the tile + a per-lane byte offset that is the same for every tile; in the ragged last
  // tile a row at or past seq_kv steps back to row seq_kv - 1.
  const int lrow = lane >> 3, lchunk = lane & 7;
  const char *kb = (const char *)(k + (int64_t)b * seq_kv * ldk + hd * 64);
  const char *vb = (const char *)(v + (int64_t)b * seq_kv * ldv + hd * 64);
  unsigned kofl[2], vofl[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * 16 + i * 8 + lrow;
    kofl[i] = (unsigned)((row * ldk + ((lchunk ^ ((row >> 1) & 7)) << 3)) * 2);
    vofl[i] = (unsigned)((row * ldv + ((lchunk ^ (((row >> 1) & 1) << 2)) << 3)) * 2);
  }
  const int64_t kstep = (int64_t)KV * ldk * 2, vstep = (int64_t)KV * ldv * 2;
  auto stage = [&](int tile, int buf) {
    char *sk = smem + buf * STAGE;
    char *sv = sk + K_BYTES;
    if ((tile + 1) * KV <= seq_kv) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        glds16(kb + kofl[i], sk + (wave * 16 + i * 8) * 128);
        glds16(vb + vofl[i], sv + (wave * 16 + i * 8) * 128);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wave * 16 + i * 8 + lrow;
        const int64_t back = max(tile * KV + row - (seq_kv - 1), 0);
        glds16(kb + kofl[i] - back * ldk * 2, sk + (wave * 16 + i * 8) * 128);
        glds16(vb + vofl[i] - back * ldv * 2, sv + (wave * 16 + i * 8) * 128);
      }
    }
    kb += kstep;
    vb += vstep;
  };

  // K operand reads: lane (r, h), k-step s, key sub-tile kt: row 32 kt + r, chunk (2 s + h) ^ ((r >> 1) & 7)
  const int kswz = (r >> 1) & 7;
  const int klane = r * 128;
  // V^T operand reads (ds_read_b64_tr_b16): lane (g = lane >> 4, q4 = (lane >> 2) & 3, pp = lane & 3) fetches the 8 bytes
  // at key 8 i + 4 (g >> 1) + q4, column 32 dt + 16 (g & 1) + 4 pp; after the transposing read the lane holds keys
  // 8 i + 4 h .. + 3 of column 32 dt + (lane & 31): the key order of the accumulator-as-operand P.
  int vlane[2];
  {
    const int g = lane >> 4, q4 = (lane >> 2) & 3, pp = lane & 3;
    const int vrow = 4 * (g >> 1) + q4, vchunk = 2 * (g & 1) + (pp >> 1), vswz = (q4 >> 1) << 2;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) vlane[dt] = vrow * 128 + (((4 * dt + vchunk) ^ vswz) << 4) + (pp & 1) * 8;
  }

  f32x16 oacc[QB][2];
  float m_run[QB], l_run[QB];
#pragma unroll
  for (int j = 0; j < QB; ++j) {
#pragma unroll
    for (int e = 0; e < 16; ++e) { oacc[j][0][e] = 0.f; oacc[j][1][e] = 0.f; }
    m_run[j] = -__builtin_inff();
    l_run[j] = 0.f;
  }

  const int ntiles = (seq_kv + KV - 1) / KV;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  int buf = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) stage(t + 1, buf ^ 1);
    const char *sk = smem + buf * STAGE;
    const char *sv = sk + K_BYTES;

    // ---- S^T = K.Q^T: 64 keys x (2 x 32) queries, fp32; every K fragment serves both query blocks
    f32x16 sacc[QB][2];
#pragma unroll
    for (int j = 0; j < QB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { sacc[j][0][e] = 0.f; sacc[j][1][e] = 0.f; }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const f16x8 kf = *(const f16x8 *)(sk + klane + kt * 32 * 128 + (((2 * s + h) ^ kswz) << 4));
#pragma unroll
        for (int j = 0; j < QB; ++j) sacc[j][kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[j][s], sacc[j][kt], 0, 0, 0);
      }

    // ---- online softmax, one query block after the other: lane (r, h) holds keys
    //      64 t + 32 kt + (e & 3) + 8 (e >> 2) + 4 h of query q0 + 32 j + r
    u32x4 pw[QB][2][2];                           // P^T as B operands: [block][kt][16-key step]
#pragma unroll
    for (int j = 0; j < QB; ++j) {
      if ((t + 1) * KV > seq_kv) {                // (only the last tile can be ragged)
        const int key0 = t * KV + 4 * h;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (key0 + 32 * kt + (e & 3) + 8 * (e >> 2) >= seq_kv) sacc[j][kt][e] = -__builtin_inff();
      }
      float mt = fmaxf(sacc[j][0][0], sacc[j][1][0]);
#pragma unroll
      for (int e = 1; e < 16; ++e) mt = fmaxf(fmaxf(mt, sacc[j][0][e]), sacc[j][1][e]);
      {                                           // the partner lane (32 away) holds the query's other 32 keys
        float ma = mt, mb = mt;                   // (two registers: the instruction swaps halves BETWEEN its operands)
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(ma), "+v"(mb));
        mt = fmaxf(ma, mb);
      }
      const float m_new = fmaxf(m_run[j], mt);    // finite from tile 0 on: every tile holds a key below seq_kv
      if (__builtin_amdgcn_ballot_w64(m_new > m_run[j]) != 0) {
        const float alpha = __builtin_amdgcn_exp2f((m_run[j] - m_new) * scale_log2e);      // (first tile: exp2(-inf) = 0)
        l_run[j] *= alpha;
#pragma unroll
        for (int e = 0; e < 16; ++e) { oacc[j][0][e] *= alpha; oacc[j][1][e] *= alpha; }
        m_run[j] = m_new;
      }
      const float nmc = -m_run[j] * scale_log2e;
      float l_tile = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const f32x2 p = {__builtin_amdgcn_exp2f(__builtin_fmaf(sacc[j][kt][e], scale_log2e, nmc)),
                           __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[j][kt][e + 1], scale_log2e, nmc))};
          l_tile += p[0] + p[1];
          pw[j][kt][e >> 3][(e & 7) >> 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(p, f16x2));
        }
      l_run[j] += l_tile;
    }

    // ---- O^T += V^T.P^T: the 8 transposing reads of one 32-column tile go out together (inline asm with its own
    //      lgkmcnt wait: for the builtin hipcc waits for the LDS-DMA of the NEXT tile); every V^T fragment serves both blocks
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const unsigned va = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)(sv + vlane[dt]);
      u32x2 vr[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vr[i]) : "v"(va), "n"(i * 8 * 128) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(vr[0]), "+v"(vr[1]), "+v"(vr[2]), "+v"(vr[3]), "+v"(vr[4]), "+v"(vr[5]), "+v"(vr[6]), "+v"(vr[7])
                   :: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const u32x4 vw = {vr[4 * kt + 2 * s][0], vr[4 * kt + 2 * s][1], vr[4 * kt + 2 * s + 1][0], vr[4 * kt + 2 * s + 1][1]};
#pragma unroll
          for (int j = 0; j < QB; ++j)
            oacc[j][dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, vw),
                                                                 __builtin_bit_cast(f16x8, pw[j][kt][s]), oacc[j][dt], 0, 0, 0);
        }
    }
    // tile t+1 has landed (this wave's pieces); every wave is done with tile t's slot before it is refilled
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    buf ^= 1;
  }

  // ---- epilogue: O^T[d][query] / l; the lane holds d = 32 dt + 8 c + 4 h .. + 3 of query q0 + 32 j + r
#pragma unroll
  for (int j = 0; j < QB; ++j) {
    const float inv = 1.0f / (l_run[j] + __shfl_xor(l_run[j], 32, 64));
    if (q0 + 32 * j + r < seq_q) {
      f16 *op = o + qrow[j] * ldo + hd * 64 + 4 * h;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          f16x4 wv;
#pragma unroll
          for (int e = 0; e < 4; ++e) wv[e] = (f16)(oacc[j][dt][4 * c + e] * inv);
          *(f16x4 *)(op + 32 * dt + 8 * c) = wv;
        }
    }
  }
}

}  // namespace

extern "C" int sp_kv_pool_f16(const void *k, const void *v, int64_t ldk, int64_t ldv, void *kp, void *vp, int64_t ldkp,
                              int64_t ldvp, int n_img, int h, int w, int c, int factor, void *stream) {
  SP_REQUIRE(k && v && kp && vp, "sp_kv_pool_f16: null pointer");
  SP_REQUIRE(factor == 2 || factor == 4, "sp_kv_pool_f16: factor %d (2 or 4)", factor);
  SP_REQUIRE(n_img > 0 && h > 0 && w > 0 && c > 0 && c % 8 == 0,
             "sp_kv_pool_f16: n_img %d, h %d, w %d must be positive and c %d a positive multiple of 8", n_img, h, w, c);
  SP_REQUIRE(h % factor == 0 && w % factor == 0, "sp_kv_pool_f16: a %d x %d grid does not divide by factor %d", h, w, factor);
  SP_REQUIRE(ldk >= c && ldv >= c && ldkp >= c && ldvp >= c,
             "sp_kv_pool_f16: row pitches (%lld, %lld, %lld, %lld) must be at least c %d", (long long)ldk, (long long)ldv,
             (long long)ldkp, (long long)ldvp, c);
  SP_REQUIRE(ldk % 8 == 0 && ldv % 8 == 0 && ldkp % 8 == 0 && ldvp % 8 == 0, "sp_kv_pool_f16: row pitches must be multiples of 8");
  SP_REQUIRE((((uintptr_t)k | (uintptr_t)v | (uintptr_t)kp | (uintptr_t)vp) & 15) == 0,
             "sp_kv_pool_f16: k, v, kp and vp must be 16-byte aligned");
  const int64_t cells = (int64_t)(h / factor) * (w / factor);            // (every product below stays inside 64 bits)
  SP_REQUIRE(cells <= 0x7fffffff && n_img * cells <= 0x7fffffff, "sp_kv_pool_f16: n_img*h*w*c too large");
  const int64_t total = n_img * cells * (c / 8);
  SP_REQUIRE((total + 255) / 256 <= 0x7fffffff, "sp_kv_pool_f16: n_img*h*w*c too large");
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  SP_CLEAR_STALE_ERROR();
  if (factor == 2)
    hipLaunchKernelGGL(kv_pool_kernel<2>, grid, dim3(256), 0, s, (const f16 *)k, (const f16 *)v, ldk, ldv, (f16 *)kp,
                       (f16 *)vp, ldkp, ldvp, h, w, c / 8, total);
  else
    hipLaunchKernelGGL(kv_pool_kernel<4>, grid, dim3(256), 0, s, (const f16 *)k, (const f16 *)v, ldk, ldv, (f16 *)kp,
                       (f16 *)vp, ldkp, ldvp, h, w, c / 8, total);
  SP_CHECK_LAUNCH("sp_kv_pool_f16");
  return SP_OK;
}

extern "C" int sp_attn_spatial_kv_f16(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk,
                                      int64_t ldv, int64_t ldo, int batch, int seq_q, int seq_kv, int heads, float scale,
                                      void *stream) {
  SP_REQUIRE(q && k && v && o, "sp_attn_spatial_kv_f16: null pointer");
  SP_REQUIRE(batch > 0 && seq_q > 0 && seq_kv > 0 && heads > 0,
             "sp_attn_spatial_kv_f16: batch %d, seq_q %d, seq_kv %d and heads %d must be positive", batch, seq_q, seq_kv, heads);
  const int64_t width = (int64_t)heads * 64;
  SP_REQUIRE(ldq >= width && ldk >= width && ldv >= width && ldo >= width,
             "sp_attn_spatial_kv_f16: row pitches (%lld, %lld, %lld, %lld) must be at least heads*64 = %lld", (long long)ldq,
             (long long)ldk, (long long)ldv, (long long)ldo, (long long)width);
  SP_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0,
             "sp_attn_spatial_kv_f16: row pitches must be multiples of 8");
  // (the LDS-DMA pieces carry 32-bit lane offsets over the 64 rows of a tile)
  SP_REQUIRE(ldk < (1ll << 24) && ldv < (1ll << 24), "sp_attn_spatial_kv_f16: row pitch too large");
  SP_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0,
             "sp_attn_spatial_kv_f16: q, k, v and o must be 16-byte aligned");
  SP_REQUIRE(scale > 0.f && scale < 3.0e38f, "sp_attn_spatial_kv_f16: scale must be positive and finite");
  const int nblk = (int)(((int64_t)seq_q + KVA_ROWS - 1) / KVA_ROWS);
  SP_REQUIRE((int64_t)batch * heads <= 0x7fffffff && (int64_t)batch * heads * nblk <= 0x7fffffff,
             "sp_attn_spatial_kv_f16: batch*heads*seq_q too large");
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(attn_kv_kernel, dim3((unsigned)(batch * heads * nblk)), dim3(256), 0, (hipStream_t)stream,
                     (const f16 *)q, (const f16 *)k, (const f16 *)v, (f16 *)o, ldq, ldk, ldv, ldo, seq_q, seq_kv, heads, nblk,
                     scale * 1.4426950408889634f);
  SP_CHECK_LAUNCH("sp_attn_spatial_kv_f16");
  return SP_OK;
}
