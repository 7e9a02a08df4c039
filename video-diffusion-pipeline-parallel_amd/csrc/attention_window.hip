// Spatial self-attention over a SLIDING WINDOW OF 8 x 8 TOKEN TILES for gfx950 (head_dim 64, fp16 in, fp32 logits and
// statistics): a frame's tokens form an h x w grid (token (y, x) is row y*w + x of its image), cut into gh x gw tiles of
// 8 x 8 tokens; a query of tile (ty, tx) attends to every key of the tile rows [y0, y0 + eh) and tile columns
// [x0, x0 + ew), eh = min(wh, gh), ew = min(ww, gw), y0 = min(max(ty - wh/2, 0), gh - eh), x0 likewise: the window is
// shifted inwards at the borders, never cut, so every query has 64*eh*ew keys and every 64 x 64 block of the score
// matrix is either dense or absent.  One entry point:
//
// sp_attn_spatial_window_f16 -- attn_window_kernel.
//  * Workgroup = 4 waves = a strip of four query tiles (ty, 4 strip .. 4 strip + 3); wave wv owns tile tx = 4 strip + wv,
//    64 queries held as two 32-query blocks (token rows 0..3 and 4..7 of the tile), as attn_kv_kernel holds its rows.  The
//    four tiles share their key tile rows; x0 does not fall as tx rises, so their key tile columns are the run
//    [x0(first tile), x0(last live tile) + ew) of at most ew + 3 columns.  Consecutive workgroups are the strips of one
//    (image, head): its K and V stay in L2 while they run.
//  * The workgroup walks that run once per key tile row.  Every 64-key tile (8 KB of K, 8 KB of V) is staged into LDS once
//    (global_load_lds_dwordx4, two 1-KiB pieces of K and of V per wave), double-buffered, one barrier per tile.  A wave
//    consumes a staged tile only if the tile's column lies in its own [x0, x0 + ew) (wave-uniform branch); it takes the
//    barrier either way.  Every consumed tile is whole and inside the window: the inner loop has no -inf, no mask, no key
//    tail.  A wave whose tx >= gw (ragged last strip) stages and takes barriers, computes and stores nothing.
//  * The gather is on the DMA's source side.  LDS tile row `row` (0..63) holds token (row >> 3, row & 7) of the tile: its
//    source is (row >> 3) * w + (row & 7) memory rows past the tile's first token.  That per-lane offset is computed once;
//    the tile base is loop-carried: + 8 rows to the next tile of a tile row, + 8 w rows (minus the run) to the next tile
//    row.  (Which key sits in which LDS row does not matter to a softmax as long as K and V agree.)  The 16-byte chunk c of
//    tile row `row` sits at chunk c ^ ((row >> 1) & 7) for K and c ^ (((row >> 1) & 1) << 2) for V, as in attention_kv.hip
//    (conflict-free ds_read_b128 / ds_read_b64_tr_b16), applied on the source side too.
//  * Q fragments and O stores use the same tile addressing: lane (r, h) of block j works on token
//    (8 ty + 4 j + (r >> 3), 8 tx + (r & 7)).
//  * Products and numerics are attn_kv_kernel's: S^T = K.Q^T and O^T += V^T.P^T on v_mfma_f32_32x32x16_f16, P in
//    registers; fp32 logits straight from the MFMA, running maximum and sum in fp32, p = exp2(s*c - m*c) with
//    c = scale*log2(e), P rounded to fp16 only as the operand of P.V, O in fp32 divided by the row sum once.
//  * No address leaves rows [b*h*w, (b+1)*h*w) and columns [64 head, 64 head + 64) of any operand.
#include "common.h"

namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int WIN_T = 8;         // tokens along each side of a tile
constexpr int WIN_TILE = 64;     // keys (and queries) per tile
constexpr int WIN_STRIP = 4;     // query tiles (waves) per workgroup
constexpr int WIN_QB = 2;        // 32-query blocks per wave

// first tile of the window of `win` tiles around tile t, shifted inwards: e = min(win, g) of g tiles
__device__ __forceinline__ int win_origin(int t, int win, int e, int g) { return min(max(t - win / 2, 0), g - e); }

// grid.x = (image, head) major, then query tile row ty, then strip
__global__ __launch_bounds__(256, 2) void attn_window_kernel(
    const f16 *__restrict__ q, const f16 *__restrict__ k, const f16 *__restrict__ v, f16 *__restrict__ o, int64_t ldq,
    int64_t ldk, int64_t ldv, int64_t ldo, int hgt, int w, int heads, int wh, int ww, int nstrip, float scale_log2e) {
  constexpr int QB = WIN_QB;
  constexpr int K_BYTES = WIN_TILE * 128, STAGE = 2 * K_BYTES;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gh = hgt / WIN_T, gw = w / WIN_T;
  const int bh = blockIdx.x / (gh * nstrip), rem = blockIdx.x - bh * (gh * nstrip);
  const int ty = rem / nstrip, strip = rem - ty * nstrip;
  const int b = bh / heads, hd = bh - b * heads;
  const int r = lane & 31, h = lane >> 5;

  const int eh = min(wh, gh), ew = min(ww, gw);
  const int tx = strip * WIN_STRIP + wave;
  const bool live = tx < gw;
  const int txc = min(tx, gw - 1);                                   // (a dead wave reads a real tile's Q and drops it)
  const int y0 = win_origin(ty, wh, eh, gh);
  const int x0 = win_origin(txc, ww, ew, gw);                        // this wave's first key tile column
  const int ux0 = win_origin(strip * WIN_STRIP, ww, ew, gw);         // the workgroup's run of key tile columns
  const int ucols = win_origin(min(strip * WIN_STRIP + WIN_STRIP - 1, gw - 1), ww, ew, gw) + ew - ux0;

  // Q fragments (B operand of S^T = K.Q^T): lane (r, h) holds Q[token][16 s + 8 h .. + 7] of token
  // (8 ty + 4 j + (r >> 3), 8 txc + (r & 7))
  const int64_t img0 = (int64_t)b * hgt * w;
  f16x8 qf[QB][4];
  int64_t qrow[QB];
#pragma unroll
  for (int j = 0; j < QB; ++j) {
    qrow[j] = img0 + (int64_t)(WIN_T * ty + 4 * j + (r >> 3)) * w + WIN_T * txc + (r & 7);
    const f16 *qp = q + qrow[j] * ldq + hd * 64 + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[j][s] = *(const f16x8 *)(qp + 16 * s);
  }

  // K/V staging: each wave moves 16 LDS rows (two token rows of the tile) of K and of V per tile, 2 + 2 LDS-DMA pieces of
  // 8 tokens x 128 bytes.  Source address = loop-carried base of the tile + a per-lane byte offset that is the same for
  // every tile (the host keeps 8*w*ld*2 below 2^32).
  const int lrow = lane >> 3, lchunk = lane & 7;
  const char *kb = (const char *)(k + (img0 + (int64_t)WIN_T * y0 * w + WIN_T * ux0) * ldk + hd * 64);
  const char *vb = (const char *)(v + (img0 + (int64_t)WIN_T * y0 * w + WIN_T * ux0) * ldv + hd * 64);
  unsigned kofl[2], vofl[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * 16 + i * 8 + lrow;                        // LDS row = token (row >> 3, row & 7) of the tile
    const int64_t src = (int64_t)(row >> 3) * w + (row & 7);
    kofl[i] = (unsigned)((src * ldk + ((lchunk ^ ((row >> 1) & 7)) << 3)) * 2);
    vofl[i] = (unsigned)((src * ldv + ((lchunk ^ (((row >> 1) & 1) << 2)) << 3)) * 2);
  }
  const int64_t kstep = (int64_t)WIN_T * ldk * 2, vstep = (int64_t)WIN_T * ldv * 2;        // next tile of the tile row
  const int64_t kdown = ((int64_t)WIN_T * w - (int64_t)WIN_T * (ucols - 1)) * ldk * 2;      // last tile of a row -> first of the next
  const int64_t vdown = ((int64_t)WIN_T * w - (int64_t)WIN_T * (ucols - 1)) * ldv * 2;
  int scol = 0;                                                      // column (within the run) of the next tile to stage
  auto stage = [&](int buf) {
    char *sk = smem + buf * STAGE;
    char *sv = sk + K_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      glds16(kb + kofl[i], sk + (wave * 16 + i * 8) * 128);
      glds16(vb + vofl[i], sv + (wave * 16 + i * 8) * 128);
    }
    if (++scol == ucols) {
      scol = 0;
      kb += kdown;
      vb += vdown;
    } else {
      kb += kstep;
      vb += vstep;
    }
  };

  // K operand reads: lane (r, h), k-step s, key sub-tile kt: row 32 kt + r, chunk (2 s + h) ^ ((r >> 1) & 7)
  const int kswz = (r >> 1) & 7;
  const int klane = r * 128;
  // V^T operand reads (ds_read_b64_tr_b16), as in attention_kv.hip: after the transposing read the lane holds keys
  // 8 i + 4 h .. + 3 of column 32 dt + (lane & 31), the key order of the accumulator-as-operand P
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

  const int ntiles = eh * ucols;
  const int c_lo = x0 - ux0, c_hi = live ? c_lo + ew : c_lo;          // this wave consumes run columns [c_lo, c_hi)
  stage(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  int buf = 0, ccol = 0;                                              // ccol: column (within the run) of the tile in `buf`
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) stage(buf ^ 1);
    if (ccol >= c_lo && ccol < c_hi) {
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

      // ---- online softmax, one query block after the other: the lane holds 32 of the tile's 64 keys for ONE query, the
      //      lane 32 away the other 32; every key is inside the window
      u32x4 pw[QB][2][2];                         // P^T as B operands: [block][kt][16-key step]
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        float mt = fmaxf(sacc[j][0][0], sacc[j][1][0]);
#pragma unroll
        for (int e = 1; e < 16; ++e) mt = fmaxf(fmaxf(mt, sacc[j][0][e]), sacc[j][1][e]);
        {
          float ma = mt, mb = mt;                 // (two registers: the instruction swaps halves BETWEEN its operands)
          asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(ma), "+v"(mb));
          mt = fmaxf(ma, mb);
        }
        const float m_new = fmaxf(m_run[j], mt);
        if (__builtin_amdgcn_ballot_w64(m_new > m_run[j]) != 0) {
          const float alpha = __builtin_amdgcn_exp2f((m_run[j] - m_new) * scale_log2e);    // (first tile: exp2(-inf) = 0)
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
      //      lgkmcnt wait); every V^T fragment serves both blocks
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
    }
    // tile t+1 has landed (this wave's pieces); every wave is done with tile t's slot before it is refilled
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    buf ^= 1;
    if (++ccol == ucols) ccol = 0;
  }

  // ---- epilogue: O^T[d][query] / l; the lane holds d = 32 dt + 8 c + 4 h .. + 3 of its query
  if (live) {
#pragma unroll
    for (int j = 0; j < QB; ++j) {
      const float inv = 1.0f / (l_run[j] + __shfl_xor(l_run[j], 32, 64));
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

extern "C" int sp_attn_spatial_window_f16(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk,
                                          int64_t ldv, int64_t ldo, int batch, int h, int w, int heads, int wh, int ww,
                                          float scale, void *stream) {
  SP_REQUIRE(q && k && v && o, "sp_attn_spatial_window_f16: null pointer");
  SP_REQUIRE(batch > 0 && heads > 0, "sp_attn_spatial_window_f16: batch %d and heads %d must be positive", batch, heads);
  SP_REQUIRE(h > 0 && w > 0 && h % WIN_T == 0 && w % WIN_T == 0,
             "sp_attn_spatial_window_f16: h %d and w %d must be positive multiples of 8 (8 x 8 token tiles)", h, w);
  SP_REQUIRE(wh > 0 && ww > 0 && wh % 2 == 1 && ww % 2 == 1,
             "sp_attn_spatial_window_f16: window (%d, %d) must be two odd positive tile counts", wh, ww);
  const int64_t width = (int64_t)heads * 64;
  SP_REQUIRE(ldq >= width && ldk >= width && ldv >= width && ldo >= width,
             "sp_attn_spatial_window_f16: row pitches (%lld, %lld, %lld, %lld) must be at least heads*64 = %lld", (long long)ldq,
             (long long)ldk, (long long)ldv, (long long)ldo, (long long)width);
  SP_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0,
             "sp_attn_spatial_window_f16: row pitches must be multiples of 8");
  // (the LDS-DMA pieces carry 32-bit lane byte offsets over the 8 token rows of a tile: 7*w + 7 memory rows)
  SP_REQUIRE(ldk < (1ll << 24) && ldv < (1ll << 24) && (int64_t)w * ldk < (1ll << 28) && (int64_t)w * ldv < (1ll << 28),
             "sp_attn_spatial_window_f16: row pitch too large (ldk, ldv below 2^24 and w*ld below 2^28)");
  SP_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0,
             "sp_attn_spatial_window_f16: q, k, v and o must be 16-byte aligned");
  SP_REQUIRE(scale > 0.f && scale < 3.0e38f, "sp_attn_spatial_window_f16: scale must be positive and finite");
  const int gh = h / WIN_T, gw = w / WIN_T, nstrip = (gw + WIN_STRIP - 1) / WIN_STRIP;
  const int64_t per_head = (int64_t)gh * nstrip;                    // (at most 2^56: every product below stays inside 64 bits)
  SP_REQUIRE((int64_t)batch * heads <= 0x7fffffff && per_head <= 0x7fffffff && (int64_t)batch * heads * per_head <= 0x7fffffff,
             "sp_attn_spatial_window_f16: batch*heads*h*w too large");
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(attn_window_kernel, dim3((unsigned)((int64_t)batch * heads * per_head)), dim3(256), 0, (hipStream_t)stream,
                     (const f16 *)q, (const f16 *)k, (const f16 *)v, (f16 *)o, ldq, ldk, ldv, ldo, h, w, heads, wh, ww, nstrip,
                     scale * 1.4426950408889634f);
  SP_CHECK_LAUNCH("sp_attn_spatial_window_f16");
  return SP_OK;
}
