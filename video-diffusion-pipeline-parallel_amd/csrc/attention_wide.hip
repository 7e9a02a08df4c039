// Fused single-head attention with a WIDE head (head_dim 128 / 256 / 512; fp16 in, fp32 logits and statistics, no
// mask): O[b] = softmax(scale * Q[b].K[b]^T).V[b] (+ bias), one kernel, no score matrix.  The VAE mid block attends with
// one head as wide as the block (512 channels in SVD's VAE); DESIGN.md section 23.
//
// At this width the constraint is the reverse of the 64-wide kernels (attention.hip, attention_long.hip): the output
// accumulator fills half the register file and one K or V tile fills 64 KB of LDS.
//
//  * Workgroup = 4 waves, one per SIMD with the whole 512-register file, one workgroup per CU.  It owns 128 consecutive
//    query rows of one image, wave w the 32 rows from 32w.  Per lane (D = 512): O^T 32 x 512 fp32 = 256 registers, the
//    wave's Q rows as MFMA operands = 128 registers' worth, loaded once (96 in registers, 32 in the LDS the tiles
//    leave: see NQL), one score tile 64 keys x 32 queries = 32.
//  * Both products run on v_mfma_f32_32x32x16_f16 in their TRANSPOSED form, S^T = K.Q^T and O^T += V^T.P^T: a lane
//    then holds 32 scores of ONE query (row statistics need one exchange with the partner lane, 32 lanes away) and
//    the score accumulator, rounded to fp16 in place, IS the B operand of the second product (no LDS round trip for P).
//    Its key order within a 16-key step (keys 4h..4h+3 and 8+4h..8+4h+3 for lane half h) is matched on the V side.
//  * V arrives row-major [keys][d]; V^T fragments (4 consecutive keys of one column per lane) come out of the
//    row-major LDS tile through ds_read_b64_tr_b16, so no V^T is ever written to HBM.
//  * LDS: ONE K tile and ONE V tile of 64 keys (2 x 64 KB at D = 512), ping-pong: the LDS-DMA of V(j) runs under
//    S^T = K(j).Q^T, the LDS-DMA of K(j+1) under the softmax and O^T += V(j)^T.P^T.  Two barriers per tile.  Pieces are
//    global_load_lds_dwordx4 of 1 KiB (whole 128-byte lines: one row at D = 512); a 16-byte chunk c of tile row `row`
//    sits at chunk c ^ swz(row), swz = ((row & 3) << 2) | ((row >> 2) & 3): 16 consecutive rows of one chunk column
//    (ds_read_b128 of K operands) and the 8 rows x 64 bytes of one transposed V read each spread over all 64 banks.
//  * Online softmax in fp32 per tile: t = s * scale*log2(e), running maximum m, p = exp2(t - m), row sum of the fp32
//    p; the 256 accumulators are rescaled only in tiles where some row's maximum rose (wave-uniform branch).  Logits
//    are never rounded to fp16 or clamped; p <= 1 is rounded to fp16 only as the MFMA operand.
//  * Tails: a key row at or beyond seq is loaded from row seq-1 (clamped address, always inside the image) and its logit
//    is set to -inf before the maximum, so its p is exactly 0; a query row at or beyond seq is computed on row seq-1
//    and not stored.  No address leaves rows [b*seq, (b+1)*seq) of any operand.
#include "common.h"

namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int WIDE_KV = 64;      // keys per tile
constexpr int WIDE_ROWS = 128;   // query rows per workgroup

// chunk swizzle of a tile row (see the head of the file)
__device__ __forceinline__ int wide_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// No packed fp32 instruction in this kernel (hipcc otherwise packs the accumulator rescale and the score scaling in pairs,
// v_pk_mul_f32 / v_pk_add_f32): the device pass compiles it with the feature off.
#if defined(__HIP_DEVICE_COMPILE__)
#define WIDE_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define WIDE_NO_PK
#endif

template <int D>
__global__ __launch_bounds__(256, 1) WIDE_NO_PK void attn_wide_kernel(
    const f16 *__restrict__ q, const f16 *__restrict__ k, const f16 *__restrict__ v, f16 *__restrict__ o, int64_t ldq,
    int64_t ldk, int64_t ldv, int64_t ldo, const float *__restrict__ bias, int seq, int nblk, float scale_log2e) {
  constexpr int KV = WIDE_KV;
  constexpr int NS = D / 16;                 // 16-deep MFMA steps of S^T = K.Q^T
  constexpr int NDT = D / 32;                // 32-column tiles of O^T
  constexpr int ROWB = 2 * D;                // bytes of a tile row
  constexpr int TILE = KV * ROWB;            // bytes of a K or V tile
  constexpr int CPR = D / 8;                 // 16-byte chunks per row
  constexpr int RPP = 64 / CPR;              // rows per 1-KiB DMA piece
  constexpr int PIECES = TILE / 1024 / 4;    // DMA pieces per wave and tile
  // Q fragments kept in LDS instead of registers (D = 512: the last 8 of 32 steps, 32 registers; the 32 KB the two tiles
  // leave): lane-private, [wave][step][lane] 16-byte pieces, read back per tile beside the K fragments (+4 % LDS reads).
  // Without it the D = 512 instantiation spills: 256 accumulators + 128 Q + P, V fragments and addresses exceed 512.
  constexpr int NQL = D == 512 ? 8 : 0, NQR = NS - NQL;
  static_assert(CPR >= 16, "the swizzle spans 16 chunks of a row");
  static_assert((KV - 8) * ROWB + 3 * 256 < 65536, "immediate offsets of the operand reads are 16 bits");
  extern __shared__ __attribute__((aligned(1024))) char wide_smem[];
  char *const sk = wide_smem, *const sv = wide_smem + TILE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int img = blockIdx.x / nblk, blk = blockIdx.x - img * nblk;
  const int64_t row0 = (int64_t)img * seq;
  const int q0 = blk * WIDE_ROWS + wave * 32;
  const int last = seq - 1;

  // Q fragments (B operand of S^T = K.Q^T): lane (r, h) holds Q[q0 + r][16 s + 8 h .. + 7]
  f16x8 qf[NQR];
  char *const sq = wide_smem + 2 * TILE + wave * (NQL * 1024) + lane * 16;
  {
    const int qrow = q0 + r < seq ? q0 + r : last;
    const f16 *qp = q + (row0 + qrow) * ldq + 8 * h;
#pragma unroll
    for (int s = 0; s < NQR; ++s) qf[s] = *(const f16x8 *)(qp + 16 * s);
#pragma unroll
    for (int s = NQR; s < NS; ++s) *(f16x8 *)(sq + (s - NQR) * 1024) = *(const f16x8 *)(qp + 16 * s);
  }

  // LDS-DMA of tile t of K or V: piece p = rows p*RPP .. of the tile, 1 KiB, lane l writes bytes 16 l .. of the piece.
  // Address = (wave-uniform base of the piece's first row, 32-bit lane offset); the lane offsets are made inside the
  // call (the empty asm keeps hipcc from holding sixteen of them per operand across the whole kernel).
  const char *const kbase = (const char *)(k + row0 * ldk);
  const char *const vbase = (const char *)(v + row0 * ldv);
  const int srow = lane / CPR, schunk = lane % CPR;
  auto stage = [&](const char *base, int64_t ld, char *dst, int t) WIDE_NO_PK {
    int sc = schunk, sr = srow;
    asm volatile("" : "+v"(sc), "+v"(sr));
#pragma unroll
    for (int c = 0; c < PIECES; ++c) {
      const int piece = wave * PIECES + c;
      const int row_u = t * KV + piece * RPP < seq ? t * KV + piece * RPP : last;      // wave-uniform
      const int row_l = t * KV + piece * RPP + sr < seq ? t * KV + piece * RPP + sr : last;
      const unsigned voff = (unsigned)(row_l - row_u) * (unsigned)(ld * 2) + ((sc ^ wide_swz(piece * RPP + sr)) << 4);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(base + (int64_t)row_u * ld * 2 + (uint64_t)voff),
                                       (__attribute__((address_space(3))) void *)(dst + piece * 1024), 16, 0, 0);
    }
  };

  // K operand reads: lane (r, h), step s, key sub-tile kt: row 32 kt + r, chunk (2 s + h) ^ swz(r); the low four chunk
  // bits take eight values over s, the rest is an immediate offset
  int kx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) kx[j] = r * ROWB + ((((2 * j) | h) ^ wide_swz(r)) << 4);
  // V^T operand reads: read i of column tile dt fetches, for lane (g = lane >> 4, q4 = (lane >> 2) & 3, pp = lane & 3),
  // the 8 bytes at key 8 i + 4 h + q4, column 32 dt + 16 (g & 1) + 4 pp; after the transposing read the lane holds
  // keys 8 i + 4 h .. + 3 of column 32 dt + (lane & 31).  Eight bases over (dt & 3, i & 1), the rest is immediate.
  unsigned vx[4][2];
  {
    const int g = lane >> 4, q4 = (lane >> 2) & 3, pp = lane & 3;
    const int cl = 2 * (g & 1) + (pp >> 1);
    const unsigned sv_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)sv;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        vx[a][b] = sv_addr + (4 * h + q4) * ROWB + (((((a ^ q4) << 2) | (cl ^ (h + 2 * b))) << 4)) + (pp & 1) * 8;
  }

  f32x16 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[dt][e] = 0.f;
  float m_run = -__builtin_inff(), l_run = 0.f;

  const int ntiles = (seq + KV - 1) / KV;
  stage(kbase, ldk, sk, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < ntiles; ++t) {
    stage(vbase, ldv, sv, t);                           // V(t) lands under the score MFMAs

    // ---- S^T = K(t).Q^T: 64 keys x 32 queries, fp32
    f32x16 sacc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { sacc[0][e] = 0.f; sacc[1][e] = 0.f; }
    // (K fragments one step ahead of their MFMAs and no further: left alone, hipcc hoists the whole tile's reads and
    // spills; the scheduling barriers keep 2 x 2 fragments live)
    f16x8 kf[2][2], ql[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) kf[0][kt] = *(const f16x8 *)(sk + kx[0] + kt * 32 * ROWB);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s + 1 < NS) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          kf[(s + 1) & 1][kt] = *(const f16x8 *)(sk + kx[(s + 1) & 7] + ((s + 1) >> 3) * 256 + kt * 32 * ROWB);
        if (s + 1 >= NQR) ql[(s + 1) & 1] = *(const f16x8 *)(sq + (s + 1 - NQR) * 1024);
      }
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[s & 1][kt], s < NQR ? qf[s] : ql[s & 1], sacc[kt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // every wave is done with K(t), every piece of V(t) has landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 < ntiles) stage(kbase, ldk, sk, t + 1);   // K(t+1) lands under the softmax and the second product

    // ---- online softmax: lane (r, h) holds keys 64 t + 32 kt + (e & 3) + 8 (e >> 2) + 4 h of query q0 + r
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[kt][e] *= scale_log2e;
    if (t == ntiles - 1 && (seq & (KV - 1)) != 0) {
      const int key0 = t * KV + 4 * h;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (key0 + 32 * kt + (e & 3) + 8 * (e >> 2) >= seq) sacc[kt][e] = -__builtin_inff();
    }
    float mt = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
    for (int e = 1; e < 16; ++e) mt = fmaxf(fmaxf(mt, sacc[0][e]), sacc[1][e]);
    {                                         // the partner lane (32 away) holds the query's other 32 keys
      float ma = mt, mb = mt;                 // (two registers: the instruction swaps halves BETWEEN its operands)
      asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(ma), "+v"(mb));
      mt = fmaxf(ma, mb);
    }
    const float m_new = fmaxf(m_run, mt);
    u32x4 pw[2][2];                                             // P^T as B operands: [kt][16-key step]
    float l_tile = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const f32x2 p = {__builtin_amdgcn_exp2f(sacc[kt][e] - m_new), __builtin_amdgcn_exp2f(sacc[kt][e + 1] - m_new)};
        l_tile += p[0] + p[1];
        pw[kt][e >> 3][(e & 7) >> 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(p, f16x2));
      }
    // some row's maximum rose: rescale what is accumulated (rare after a few tiles).  Behind the exponentials, where the
    // scores are dead, and one 16-register tile at a time: the 256 accumulators leave no room for more.
    if (__builtin_amdgcn_ballot_w64(m_new > m_run) != 0) {
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[dt][e] *= alpha;
        __builtin_amdgcn_sched_barrier(0);
      }
      m_run = m_new;
    }
    l_run += l_tile;

    // ---- O^T += V(t)^T.P^T: per 32-column tile eight transposing reads (inline asm: for the builtin hipcc waits for the
    // LDS-DMA in flight) and four MFMAs; the reads of tile dt + 1 are issued ahead of the MFMAs of tile dt
    u32x2 vr[2][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vr[0][i]) : "v"(vx[0][i & 1]), "n"(i * 8 * ROWB) : "memory");
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      u32x2(&vc)[8] = vr[dt & 1];
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(vc[0]), "+v"(vc[1]), "+v"(vc[2]), "+v"(vc[3]), "+v"(vc[4]), "+v"(vc[5]), "+v"(vc[6]), "+v"(vc[7])
                   :: "memory");
      if (dt + 1 < NDT) {
        u32x2(&vn)[8] = vr[(dt + 1) & 1];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
                       : "=v"(vn[i])
                       : "v"(vx[(dt + 1) & 3][i & 1]), "n"(i * 8 * ROWB + ((dt + 1) >> 2) * 256)
                       : "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const u32x4 vw = {vc[2 * ks][0], vc[2 * ks][1], vc[2 * ks + 1][0], vc[2 * ks + 1][1]};
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, vw),
                                                          __builtin_bit_cast(f16x8, pw[ks >> 1][ks & 1]), oacc[dt], 0, 0, 0);
      }
    }

    // every wave is done with V(t), every piece of K(t+1) has landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // ---- epilogue: O^T / l (+ bias) to fp16.  The lane holds columns 32 dt + 8 c + 4 h .. + 3 (c = e >> 2) of query
  // q0 + r; it trades one group of four with its partner lane per pair of groups and stores 16 bytes:
  // columns 32 dt + 16 cp + 8 h .. + 7.
  // (ds_bpermute: the value of lane ^ 32)
  const int partner = (lane ^ 32) << 2;
  const float inv = 1.0f / (l_run + __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(partner, __builtin_bit_cast(int, l_run))));
  const bool live = q0 + r < seq;
  f16 *const op = o + (row0 + (live ? q0 + r : last)) * ldo + 8 * h;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    u32x2 pk[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 val = {oacc[dt][4 * c] * inv, oacc[dt][4 * c + 1] * inv, oacc[dt][4 * c + 2] * inv, oacc[dt][4 * c + 3] * inv};
      if (bias) val += *(const f32x4 *)(bias + 32 * dt + 8 * c + 4 * h);
      const f16x4 w = __builtin_convertvector(val, f16x4);
      pk[c] = __builtin_bit_cast(u32x2, w);
    }
#pragma unroll
    for (int cp = 0; cp < 2; ++cp) {
      const u32x2 mine = h ? pk[2 * cp + 1] : pk[2 * cp], send = h ? pk[2 * cp] : pk[2 * cp + 1];
      const u32x2 got = {(unsigned)__builtin_amdgcn_ds_bpermute(partner, (int)send[0]),
                         (unsigned)__builtin_amdgcn_ds_bpermute(partner, (int)send[1])};
      const u32x4 w = h ? (u32x4){got[0], got[1], mine[0], mine[1]} : (u32x4){mine[0], mine[1], got[0], got[1]};
      if (live) *(u32x4 *)(op + 32 * dt + 16 * cp) = w;
    }
  }
}

template <int D>
int wide_launch(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                const float *bias, int batch, int seq, float scale, hipStream_t s) {
  static bool attr_set[SP_MAX_DEVICES];
  constexpr int lds = 2 * WIDE_KV * D * 2 + (D == 512 ? 32768 : 0);   // K tile, V tile, (D = 512) eight Q steps
  static_assert(lds <= 160 * 1024, "LDS per workgroup");
  if (int rc = sp_ensure_dyn_lds((const void *)attn_wide_kernel<D>, lds, attr_set, "sp_attn_wide_f16")) return rc;
  const int nblk = (seq + WIDE_ROWS - 1) / WIDE_ROWS;
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(attn_wide_kernel<D>, dim3((unsigned)(batch * nblk)), dim3(256), lds, s, (const f16 *)q, (const f16 *)k,
                     (const f16 *)v, (f16 *)o, ldq, ldk, ldv, ldo, bias, seq, nblk, scale * 1.4426950408889634f);
  SP_CHECK_LAUNCH("sp_attn_wide_f16");
  return SP_OK;
}

}  // namespace

extern "C" int sp_attn_wide_f16(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk, int64_t ldv,
                                int64_t ldo, const float *bias, int batch, int seq, int head_dim, float scale,
                                void *stream) {
  SP_REQUIRE(q && k && v && o, "sp_attn_wide_f16: null pointer");
  SP_REQUIRE(head_dim == 128 || head_dim == 256 || head_dim == 512,
             "sp_attn_wide_f16: head_dim %d (128, 256 or 512; 64-wide heads: sp_attn_spatial_f16)", head_dim);
  SP_REQUIRE(batch > 0 && seq > 0, "sp_attn_wide_f16: batch %d and seq %d must be positive", batch, seq);
  SP_REQUIRE(ldq >= head_dim && ldk >= head_dim && ldv >= head_dim && ldo >= head_dim,
             "sp_attn_wide_f16: row pitches (%lld, %lld, %lld, %lld) must be at least head_dim %d", (long long)ldq,
             (long long)ldk, (long long)ldv, (long long)ldo, head_dim);
  SP_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "sp_attn_wide_f16: row pitches must be multiples of 8");
  // (the LDS-DMA pieces carry 32-bit lane offsets over up to four rows)
  SP_REQUIRE(ldk < (1ll << 28) && ldv < (1ll << 28), "sp_attn_wide_f16: row pitch too large");
  SP_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)bias) & 15) == 0,
             "sp_attn_wide_f16: q, k, v, o and bias must be 16-byte aligned");
  SP_REQUIRE(scale > 0.f && scale < 3.0e38f, "sp_attn_wide_f16: scale must be positive and finite");
  SP_REQUIRE((int64_t)batch * ((seq + WIDE_ROWS - 1) / WIDE_ROWS) <= 0x7fffffff, "sp_attn_wide_f16: batch*seq too large");
  hipStream_t s = (hipStream_t)stream;
  switch (head_dim) {
    case 128: return wide_launch<128>(q, k, v, o, ldq, ldk, ldv, ldo, bias, batch, seq, scale, s);
    case 256: return wide_launch<256>(q, k, v, o, ldq, ldk, ldv, ldo, bias, batch, seq, scale, s);
    default: return wide_launch<512>(q, k, v, o, ldq, ldk, ldv, ldo, bias, batch, seq, scale, s);
  }
}
