// Temporal self-attention for LONG clips on gfx950: sequences of 33 .. 128 tokens that run across frames, head_dim 64,
// fp16 in / fp32 accumulate, no mask, no dropout.  attn_temporal_kernel (attention.hip) holds a whole sequence in
// registers (Q and K fragments from global memory, NT x NT score tiles) and stops at 32 frames; this kernel splits the
// work differently and keeps that kernel's arithmetic.
//
// attn_temporal_long_kernel<NKT> -- NKT key tiles of 16 frames (Fpad = 16 NKT >= frames): 4, 6, 8 for <= 64, 96, 128.
//   Work split.  One wave owns one (video, pixel, head) problem; a workgroup is TL_WAVES = 2 waves with private LDS
//   regions and no barrier.  The wave loops over query blocks of 32 frames (two 16-row MFMA tiles) against all keys.
//   LDS per wave.  [K: Fpad rows x 128 B][V: Fpad rows x 128 B][O block: 32 rows x 128 B]; at 128 frames 36 KB, 72 KB per
//   workgroup, so two workgroups share a CU's 160 KB.  K and V are brought in once, before the query loop, by LDS-DMA
//   (global_load_lds_dwordx4, 8 rows per instruction); rows at or beyond `frames` come from the zero page.  K and V are
//   read by every query block, so O has a tile of its own and no slice of K or V is ever overwritten.
//   K operand.  K is the MFMA A operand: lane (fr = lane & 15, fq = lane >> 4) reads the 16 bytes K[16 kt + fr][32 s + 8 fq ..]
//   -- sixteen lanes, rows 128 bytes apart, one chunk: one bank group.  The 16-byte chunk index is XORed with the row,
//   position = chunk ^ (row & 7); each lane applies it on the SOURCE side of the LDS-DMA (LDS position `lchunk` of row r
//   receives source chunk lchunk ^ (r & 7)), as attn_spatial_kernel does.  V keeps its natural layout and is read by
//   ds_read_b64_tr_b16 as the B operand of P.V, as in attn_temporal_kernel.
//   Scores.  S^T[kt][qt] = K.Q^T on v_mfma_f32_16x16x32_f16: column = query frame (lane & 15) of tile qt, rows = keys
//   16 kt + 4 fq + e.  The whole key row of a query block stays in registers: NKT x 2 x 4 <= 64 accumulator registers; the
//   tile loops are unrolled at compile time.  Q fragments (B operand) come straight from global memory, per block.
//   Softmax.  Two passes, no online rescale -- attn_temporal_kernel's contract: keys >= frames masked, row maximum (two
//   __shfl_xor steps across the four lane groups), p = exp2(s c - max c) with c = scale log2 e, fp32 sum, P / l rounded
//   to fp16, P.V on v_mfma_f32_16x16x16f16 with fp32 accumulation, one rounding to fp16.
//   Output.  O of a block -> the wave's O tile -> 16-byte row stores; a query frame >= frames is never stored.
//   The last workgroup's dead wave clamps to the last problem (EXEC stays full for the transposed reads) and stores nothing.
#include "common.h"

namespace {

typedef short v4i16 __attribute__((__vector_size__(8)));

__device__ __forceinline__ f16x4 lds_tr16(const char *p) {
  v4i16 raw = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16 *)p);
  return __builtin_bit_cast(f16x4, raw);
}

constexpr float NEG_BIG = -3.0e38f;
constexpr int TL_WAVES = 2;                    // waves (= problems) per workgroup
constexpr int TL_QB = 32;                      // query frames per block
constexpr int TL_O_BYTES = TL_QB * 128;        // O tile of one wave

constexpr int tl_wave_bytes(int nkt) { return 2 * nkt * 16 * 128 + TL_O_BYTES; }

template <int NKT>
__global__ __launch_bounds__(TL_WAVES * 64) void attn_temporal_long_kernel(
    const f16 *__restrict__ q, const f16 *__restrict__ k, const f16 *__restrict__ v, f16 *__restrict__ o,
    int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int frames, int64_t hw, int heads,
    int64_t nproblems, float scale_log2e, const char *__restrict__ zero) {
  constexpr int KV_BYTES = NKT * 16 * 128;             // K (and V) of one problem: [16 NKT][64] f16
  extern __shared__ __attribute__((aligned(1024))) char tl_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int64_t prob = (int64_t)blockIdx.x * TL_WAVES + wave;
  const bool live = prob < nproblems;
  if (!live) prob = nproblems - 1;                     // keep EXEC full for the transposed reads
  const int hd = (int)(prob % heads);
  const int64_t bp = prob / heads;                     // b*hw + p
  const int64_t b = bp / hw, p = bp - b * hw;
  const int64_t tok0 = b * frames * hw + p;            // row of frame 0
  char *ks = tl_smem + wave * tl_wave_bytes(NKT);
  char *vs = ks + KV_BYTES;
  char *os = vs + KV_BYTES;

  const int fr = lane & 15, fq = lane >> 4;
  const int lrow = lane >> 3, lchunk = lane & 7;
  // ---- K (chunk-swizzled) and V -> LDS, once; zero rows past `frames`.  Instruction i moves frames 8i .. 8i+7 (frame & 7
  // == lrow); the per-lane source walks 8 frames per step and is followed only while the frame exists.
  {
    const char *ksrc = (const char *)(k + (tok0 + lrow * hw) * ldk + hd * 64 + ((lchunk ^ lrow) << 3));
    const char *vsrc = (const char *)(v + (tok0 + lrow * hw) * ldv + hd * 64 + (lchunk << 3));
    const char *zsrc = zero + lchunk * 16;
    const int64_t kstep = 8 * hw * ldk * 2, vstep = 8 * hw * ldv * 2;
#pragma nounroll
    for (int i = 0; i < 2 * NKT; ++i) {            // (rolled: unrolled, its 2 NKT lane masks and row offsets spill SGPRs)
      const bool ok = i * 8 + lrow < frames;
      glds16(ok ? ksrc : zsrc, ks + i * 1024);
      glds16(ok ? vsrc : zsrc, vs + i * 1024);
      ksrc += kstep;
      vsrc += vstep;
    }
  }
  // lane parts of the operand addresses
  const char *kread = ks + fr * 128;                   // + kt*2048 + (((4s + fq) ^ (fr & 7)) << 4)
  int kchunk[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) kchunk[s] = ((4 * s + fq) ^ (fr & 7)) << 4;
  const char *vread = vs + (4 * fq + (fr >> 2)) * 128 + (4 * (fr & 3)) * 2;   // + kt*2048 + dt*32
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  const int nqb = (frames + TL_QB - 1) / TL_QB;
#pragma nounroll
  for (int qb = 0; qb < nqb; ++qb) {
    const int q0 = qb * TL_QB;
    // ---- Q fragments of the block straight from global memory
    f16x8 qf[2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int f = q0 + qt * 16 + fr;
      const bool ok = f < frames;
      const f16 *qp = ok ? q + (tok0 + (int64_t)f * hw) * ldq + hd * 64 + 8 * fq : (const f16 *)zero;
#pragma unroll
      for (int s = 0; s < 2; ++s) qf[qt][s] = *(const f16x8 *)(qp + (ok ? 32 * s : 0));
    }
    // ---- S^T[kt][qt]: col = query frame (fr) of tile qt, row = key 16kt + 4fq + e
    f32x4 sacc[NKT][2];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f16x8 kf[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) kf[s] = *(const f16x8 *)(kread + kt * 2048 + kchunk[s]);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        sacc[kt][qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s)
          sacc[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[s], qf[qt][s], sacc[kt][qt], 0, 0, 0);
      }
    }
    // ---- softmax over keys for both query columns, P normalised in fp32 and rounded to fp16
    f16x4 pf[2][NKT];   // [qt][kt]
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float mx = NEG_BIG;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = 16 * kt + 4 * fq + e;
          if (key >= frames) sacc[kt][qt][e] = NEG_BIG;
          mx = fmaxf(mx, sacc[kt][qt][e]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mb = mx * scale_log2e;
      float sum = 0.f;
      float pv[NKT][4];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pv[kt][e] = __builtin_amdgcn_exp2f(sacc[kt][qt][e] * scale_log2e - mb);
          sum += pv[kt][e];
        }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[qt][kt][e] = (f16)(pv[kt][e] * inv);
    }
    // ---- O[qt][dt] = sum_kt P[qt][kt] . V[kt][dt]   (B operand by transposed LDS read)
    f32x4 oacc[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oacc[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f16x4 vf = lds_tr16(vread + kt * 2048 + dt * 32);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
          oacc[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x16f16(pf[qt][kt], vf, oacc[qt][dt], 0, 0, 0);
      }
    // ---- O block -> the wave's own O tile -> 16-byte row stores (K and V stay intact for the next block)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          *(f16 *)(os + (16 * qt + 4 * fq + e) * 128 + (16 * dt + fr) * 2) = (f16)oacc[qt][dt][e];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < TL_QB / 8; ++i) {
      const int f = q0 + i * 8 + lrow;
      const f16x8 w = *(const f16x8 *)(os + (i * 8 + lrow) * 128 + lchunk * 16);
      if (live && f < frames) *(f16x8 *)(o + (tok0 + (int64_t)f * hw) * ldo + hd * 64 + lchunk * 8) = w;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tile is read out before the next block writes it
  }
}

template <int NKT>
int temporal_long_launch(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk, int64_t ldv,
                         int64_t ldo, int frames, int64_t hw, int heads, int64_t nprob, float scale, const void *zero_page,
                         hipStream_t s) {
  static bool attr_set[SP_MAX_DEVICES];
  constexpr int lds = TL_WAVES * tl_wave_bytes(NKT);
  static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
  if (int rc = sp_ensure_dyn_lds((const void *)attn_temporal_long_kernel<NKT>, lds, attr_set, "sp_attn_temporal_long_f16"))
    return rc;
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(attn_temporal_long_kernel<NKT>, dim3((unsigned)((nprob + TL_WAVES - 1) / TL_WAVES)), dim3(TL_WAVES * 64),
                     lds, s, (const f16 *)q, (const f16 *)k, (const f16 *)v, (f16 *)o, ldq, ldk, ldv, ldo, frames, hw, heads,
                     nprob, scale * 1.4426950408889634f, (const char *)zero_page);
  SP_CHECK_LAUNCH("sp_attn_temporal_long_f16");
  return SP_OK;
}

}  // namespace

extern "C" int sp_attn_temporal_long_f16(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk,
                                         int64_t ldv, int64_t ldo, int batch, int frames, int64_t hw, int heads,
                                         float scale, const void *zero_page, void *stream) {
  SP_REQUIRE(q && k && v && o && zero_page, "sp_attn_temporal_long_f16: null pointer");
  SP_REQUIRE(frames >= 33 && frames <= 128,
             "sp_attn_temporal_long_f16: unsupported shape (frames=%d must be in [33,128]; up to 32: sp_attn_temporal_f16)",
             frames);
  SP_REQUIRE(batch > 0 && hw > 0 && heads > 0, "sp_attn_temporal_long_f16: batch %d, hw %lld and heads %d must be positive",
             batch, (long long)hw, heads);
  const int64_t c = (int64_t)heads * 64;
  SP_REQUIRE(ldq >= c && ldk >= c && ldv >= c && ldo >= c,
             "sp_attn_temporal_long_f16: row pitches (%lld, %lld, %lld, %lld) must be at least heads*64 = %lld", (long long)ldq,
             (long long)ldk, (long long)ldv, (long long)ldo, (long long)c);
  SP_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0,
             "sp_attn_temporal_long_f16: row pitches must be multiples of 8");
  SP_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)zero_page) & 15) == 0,
             "sp_attn_temporal_long_f16: q, k, v, o and zero_page must be 16-byte aligned");
  SP_REQUIRE(scale > 0.f && scale < 3.0e38f, "sp_attn_temporal_long_f16: scale must be positive and finite");
  // problems = batch*hw*heads, two per workgroup of a one-dimensional grid; rows = batch*frames*hw
  SP_REQUIRE(hw <= (1ll << 31) / ((int64_t)batch * heads) && hw <= (1ll << 40) / ((int64_t)batch * frames),
             "sp_attn_temporal_long_f16: batch*hw*heads too large");
  const int64_t nprob = (int64_t)batch * hw * heads;
  hipStream_t s = (hipStream_t)stream;
  if (frames <= 64)
    return temporal_long_launch<4>(q, k, v, o, ldq, ldk, ldv, ldo, frames, hw, heads, nprob, scale, zero_page, s);
  if (frames <= 96)
    return temporal_long_launch<6>(q, k, v, o, ldq, ldk, ldv, ldo, frames, hw, heads, nprob, scale, zero_page, s);
  return temporal_long_launch<8>(q, k, v, o, ldq, ldk, ldv, ldo, frames, hw, heads, nprob, scale, zero_page, s);
}
