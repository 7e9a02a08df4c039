// Pictures in: a baseline JPEG file's entropy-coded segment, uploaded as it is, becomes (h, w, 3) uint8 RGB on the device.
// The host walks the markers (models/image_io.py: parse_jpeg) and makes a plan (sp_jpeg_decode_plan: sizes, selectors, derived
// Huffman tables); everything from the compressed bytes on is here.  include/svdpipe.h fixes the rules, jpeg_decode_core.h holds
// the lane's decode step, the guarded store and the integer pixel arithmetic, shared with tools/jpeg_decode_hostcheck.cpp.
//
//   sp_jpeg_decode_split        : jd_count_kernel (a workgroup per 4 KiB: bytes kept and RSTn markers), jd_scan_bytes_kernel (one
//                                 workgroup: exclusive scan of both counts over the workgroups), jd_compact_kernel (the clean
//                                 bytes at their scanned positions, the start of interval k + 1 at marker k, the order of the
//                                 markers checked), jd_intervals_kernel (subsequences per interval and their exclusive scan).
//   sp_jpeg_decode_sync         : jd_pass_kernel, `passes` times.  A lane per subsequence, the four tables in LDS.  A pass
//                                 reads the records of the pass before it and writes its own (two buffers), so a pass is a
//                                 function of the one before and the count of passes is the same on every run.  A lane whose
//                                 start did not change copies its record; one that meets an invalid symbol notes it in its
//                                 record and goes on (jd_step), so that lanes started at a wrong bit still find the true walk.
//                                 A pass leaves at once when the pass before changed no record.
//   sp_jpeg_decode_coefficients : only once the fixed point is reached: jd_lane_sum_kernel / jd_scan_small_kernel /
//                                 jd_lane_first_kernel (exclusive scan of the lanes' block counts), jd_check_kernel (every
//                                 interval's chain must come to its MCUs x blocks per MCU), jd_write_kernel (the lanes walk
//                                 once more and store), jd_dc_kernel twice around jd_dc_carry_kernel (DC differences -> values:
//                                 a segmented scan over MCUs, segments the restart intervals, in 32 bits, clamped to int16).
//   sp_jpeg_decode_pixels       : jd_idct_kernel (a thread per block: dequantise, jidctint, planes of whole MCUs),
//                                 jd_rgb_kernel (a thread per pixel: triangle-filter upsampling at the component's own size,
//                                 YCbCr -> RGB, crop).
// Every kernel after the split leaves at once while the error word is set, so nothing is decoded from positions a broken
// stream gave; every position is clamped to the clean stream's length besides.
#include <string.h>
#include "common.h"
#include "jpeg_decode_core.h"

namespace {

typedef unsigned char u8;
typedef unsigned int u32;

__device__ __forceinline__ u32 wave_incl_scan(u32 v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive scan over the 256 threads of a workgroup; *total is the sum.  wsum: 4 words of LDS.
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32 *wsum, u32 *total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u32 inc = wave_incl_scan(v);
  __syncthreads();
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  u32 base = 0;
  for (int i = 0; i < wv; ++i) base += wsum[i];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return base + inc - v;
}

// a[0 .. n) -> its exclusive scan in place, by one workgroup of 256; the sum (returned to every thread)
__device__ u32 scan_array_inplace(u32 *a, int n, u32 *wsum) {
  u32 carry = 0;
  for (int b0 = 0; b0 < n; b0 += 256) {
    const int i = b0 + (int)threadIdx.x;
    const u32 v = i < n ? a[i] : 0u;
    u32 total;
    const u32 ex = block_excl_scan(v, wsum, &total);
    if (i < n) a[i] = carry + ex;
    carry += total;
  }
  return carry;
}

constexpr int BYTES_PER_THREAD = JD_BYTES_PER_BLOCK / 256;

__global__ __launch_bounds__(256) void jd_count_kernel(const u8 *__restrict__ seg, int len, u32 *__restrict__ blk_keep,
                                                       u32 *__restrict__ blk_mark, int *__restrict__ meta) {
  __shared__ u32 wsum[4];
  const int64_t i0 = (int64_t)blockIdx.x * JD_BYTES_PER_BLOCK + (int64_t)threadIdx.x * BYTES_PER_THREAD;
  u32 keep = 0, mark = 0, bad = 0;
  if (i0 < len) {
    int prev = i0 > 0 ? seg[i0 - 1] : 0, b = seg[i0];
    for (int k = 0; k < BYTES_PER_THREAD && i0 + k < len; ++k) {
      const int next = i0 + k + 1 < len ? seg[i0 + k + 1] : -1;
      const int c = jd_classify(prev, b, next);
      keep += c & 1, mark += (c >> 1) & 1, bad |= (u32)c >> 2;
      prev = b, b = next;
    }
  }
  u32 total;
  block_excl_scan(keep, wsum, &total);
  if (threadIdx.x == 0) blk_keep[blockIdx.x] = total;
  block_excl_scan(mark, wsum, &total);
  if (threadIdx.x == 0) blk_mark[blockIdx.x] = total;
  if (bad) atomicOr(meta + JD_M_ERROR, JD_E_MARKER);
}

__global__ __launch_bounds__(256) void jd_scan_bytes_kernel(u32 *__restrict__ blk_keep, u32 *__restrict__ blk_mark, int blocks,
                                                            int n_iv, u32 *__restrict__ iv_start, int *__restrict__ meta) {
  __shared__ u32 wsum[4];
  const u32 clean = scan_array_inplace(blk_keep, blocks, wsum);
  const u32 marks = scan_array_inplace(blk_mark, blocks, wsum);
  if (threadIdx.x == 0) {
    meta[JD_M_CLEAN] = (int)clean, meta[JD_M_MARKERS] = (int)marks;
    iv_start[0] = 0, iv_start[n_iv] = clean;
    if (marks != (u32)(n_iv - 1)) atomicOr(meta + JD_M_ERROR, JD_E_RST_COUNT);
  }
}

__global__ __launch_bounds__(256) void jd_compact_kernel(const u8 *__restrict__ seg, int len, const u32 *__restrict__ blk_keep,
                                                         const u32 *__restrict__ blk_mark, int n_iv, u8 *__restrict__ clean,
                                                         u32 *__restrict__ iv_start, int *__restrict__ meta) {
  __shared__ u32 wsum[4];
  const int64_t i0 = (int64_t)blockIdx.x * JD_BYTES_PER_BLOCK + (int64_t)threadIdx.x * BYTES_PER_THREAD;
  u32 keep = 0, mark = 0;
  int cls[BYTES_PER_THREAD], val[BYTES_PER_THREAD], code[BYTES_PER_THREAD];
#pragma unroll
  for (int k = 0; k < BYTES_PER_THREAD; ++k) cls[k] = 0, val[k] = 0, code[k] = 0;
  if (i0 < len) {
    int prev = i0 > 0 ? seg[i0 - 1] : 0, b = seg[i0];
#pragma unroll
    for (int k = 0; k < BYTES_PER_THREAD; ++k) {
      if (i0 + k < len) {
        const int next = i0 + k + 1 < len ? seg[i0 + k + 1] : -1;
        cls[k] = jd_classify(prev, b, next), val[k] = b, code[k] = next;
        keep += cls[k] & 1, mark += (cls[k] >> 1) & 1;
        prev = b, b = next;
      }
    }
  }
  u32 total;
  u32 at = blk_keep[blockIdx.x] + block_excl_scan(keep, wsum, &total);
  u32 mk = blk_mark[blockIdx.x] + block_excl_scan(mark, wsum, &total);
  bool order = true;
#pragma unroll
  for (int k = 0; k < BYTES_PER_THREAD; ++k) {
    if (cls[k] & 1) {
      if (at < (u32)len) clean[at] = (u8)val[k];             // (kept bytes never outnumber the segment's)
      ++at;
    } else if (cls[k] & 2) {
      order = order && code[k] == 0xD0 + (int)(mk & 7);
      if (mk + 1 < (u32)n_iv) iv_start[mk + 1] = at;
      ++mk;
    }
  }
  if (!order) atomicOr(meta + JD_M_ERROR, JD_E_RST_ORDER);
}

constexpr int IV_PER_THREAD = 8;

// one workgroup: subsequences of every interval, their exclusive scan, the total and the longest
__global__ __launch_bounds__(256) void jd_intervals_kernel(const u32 *__restrict__ iv_start, int n_iv, int subseq_bits, int max_sub,
                                                           u32 *__restrict__ sub_first, int *__restrict__ meta) {
  __shared__ u32 wsum[4];
  __shared__ u32 longest;
  if (threadIdx.x == 0) longest = 0;
  __syncthreads();
  if (meta[JD_M_ERROR]) {
    if (threadIdx.x == 0) meta[JD_M_SUBS] = 0, meta[JD_M_LONGEST] = 0;
    return;
  }
  const u32 clean = (u32)meta[JD_M_CLEAN];
  u32 carry = 0, mine_max = 0;
  for (int b0 = 0; b0 < n_iv; b0 += 256 * IV_PER_THREAD) {
    const int k0 = b0 + (int)threadIdx.x * IV_PER_THREAD;
    u32 ns[IV_PER_THREAD], sum = 0;
#pragma unroll
    for (int j = 0; j < IV_PER_THREAD; ++j) {
      ns[j] = 0;
      if (k0 + j < n_iv) {
        const u32 lo = min(iv_start[k0 + j], clean), hi = min(iv_start[k0 + j + 1], clean);
        const u32 bits = hi > lo ? 8u * (hi - lo) : 0u;
        ns[j] = (bits + (u32)subseq_bits - 1) / (u32)subseq_bits;
        mine_max = max(mine_max, ns[j]);
      }
      sum += ns[j];
    }
    u32 total;
    u32 at = carry + block_excl_scan(sum, wsum, &total);
#pragma unroll
    for (int j = 0; j < IV_PER_THREAD; ++j)
      if (k0 + j < n_iv) sub_first[k0 + j] = at, at += ns[j];
    carry += total;
  }
  atomicMax(&longest, mine_max);
  __syncthreads();
  if (threadIdx.x == 0) {
    sub_first[n_iv] = carry;
    meta[JD_M_SUBS] = (int)min(carry, (u32)max_sub), meta[JD_M_LONGEST] = (int)longest;   // (carry <= max_sub by its definition)
  }
}

// the interval that holds subsequence g: the last k with sub_first[k] <= g
__device__ __forceinline__ int interval_of(const u32 *__restrict__ sub_first, int n_iv, u32 g) {
  int lo = 0, hi = n_iv - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sub_first[mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void load_huff(JdHuff *dst, const JdPlan *__restrict__ plan) {
  const u32 *src = (const u32 *)plan->t.huff;
  u32 *d = (u32 *)dst;
  for (int i = threadIdx.x; i < (int)(4 * sizeof(JdHuff) / 4); i += 256) d[i] = src[i];
  __syncthreads();
}

struct LaneSpan {
  u32 bit0, end_bits, j, first_sub;
  int k;
};

__device__ __forceinline__ LaneSpan lane_span(const u32 *__restrict__ iv_start, const u32 *__restrict__ sub_first, int n_iv, u32 clean,
                                              u32 g) {
  LaneSpan s;
  s.k = interval_of(sub_first, n_iv, g);
  s.first_sub = sub_first[s.k];
  s.j = g - s.first_sub;
  s.bit0 = 8u * min(iv_start[s.k], clean), s.end_bits = 8u * min(iv_start[s.k + 1], clean);
  return s;
}

__global__ __launch_bounds__(256) void jd_pass_kernel(JdParams p, const JdPlan *__restrict__ plan, const u32 *__restrict__ words,
                                                      const u32 *__restrict__ iv_start, const u32 *__restrict__ sub_first,
                                                      const JdRec *__restrict__ rec_in, JdRec *__restrict__ rec_out, int pass,
                                                      int *__restrict__ meta) {
  __shared__ JdHuff huff[4];
  if (meta[JD_M_ERROR]) return;
  const u32 g = blockIdx.x * 256u + threadIdx.x;
  if (meta[JD_M_FIXED] || (pass > 0 && meta[JD_M_CHANGED + (pass + 2) % 3] == 0)) {
    if (g == 0) meta[JD_M_FIXED] = 1;
    return;
  }
  const u32 subs = (u32)meta[JD_M_SUBS];
  if (blockIdx.x * 256u >= subs) return;
  if (g == 0) meta[JD_M_PASSES] = pass + 1, meta[JD_M_CHANGED + (pass + 1) % 3] = 0;
  load_huff(huff, plan);
  int changed = 0;
  if (g < subs) {
    const LaneSpan s = lane_span(iv_start, sub_first, p.n_iv, (u32)meta[JD_M_CLEAN], g);
    const JdRec mine = pass > 0 ? rec_in[g] : JdRec{};
    const JdRec prev = pass > 0 && s.j > 0 ? rec_in[g - 1] : JdRec{};
    JdRec out;
    changed = jd_lane_pass(words, s.bit0, s.end_bits, s.j, pass, huff, &p, &prev, &mine, &out);
    rec_out[g] = out;
  }
  const unsigned long long any = __ballot(changed);
  if ((threadIdx.x & 63) == 0 && any) atomicAdd(meta + JD_M_CHANGED + pass % 3, (int)__popcll(any));
}

// The records of the last pass that ran: its starts are the exits of the pass before, which it found unchanged, so they are
// the true ones (the other buffer has the same exits, but may have reached them from older starts).
__device__ __forceinline__ const JdRec *final_rec(const JdRec *rec0, const JdRec *rec1, const int *__restrict__ meta) {
  return ((meta[JD_M_PASSES] - 1) & 1) ? rec1 : rec0;
}

// every kernel behind the synchronisation passes: true once a pass changed nothing, and no error is set
__device__ __forceinline__ bool settled(const int *__restrict__ meta, int last_pass) {
  return !meta[JD_M_ERROR] && (meta[JD_M_FIXED] || meta[JD_M_CHANGED + last_pass % 3] == 0);
}

constexpr int LANES_PER_THREAD = JD_LANES_PER_PART / 256;

__global__ __launch_bounds__(256) void jd_lane_sum_kernel(const JdRec *__restrict__ rec0, const JdRec *__restrict__ rec1,
                                                          u32 *__restrict__ lane_part, int last_pass, int *__restrict__ meta) {
  __shared__ u32 wsum[4];
  if (!settled(meta, last_pass)) return;
  const JdRec *rec = final_rec(rec0, rec1, meta);
  const u32 subs = (u32)meta[JD_M_SUBS];
  const u32 g0 = blockIdx.x * (u32)JD_LANES_PER_PART + threadIdx.x * (u32)LANES_PER_THREAD;
  u32 sum = 0, bad = 0;
  for (int j = 0; j < LANES_PER_THREAD; ++j)
    if (g0 + j < subs) sum += rec[g0 + j].nblk, bad |= rec[g0 + j].err;
  u32 total;
  block_excl_scan(sum, wsum, &total);
  if (threadIdx.x == 0) lane_part[blockIdx.x] = total;
  if (bad) atomicOr(meta + JD_M_ERROR, JD_E_CODE);
}

__global__ __launch_bounds__(256) void jd_scan_small_kernel(u32 *__restrict__ a, int n, int last_pass, const int *__restrict__ meta) {
  __shared__ u32 wsum[4];
  if (!(meta[JD_M_FIXED] || meta[JD_M_CHANGED + last_pass % 3] == 0)) return;
  const u32 total = scan_array_inplace(a, n, wsum);
  if (threadIdx.x == 0) a[n] = total;
}

__global__ __launch_bounds__(256) void jd_lane_first_kernel(const JdRec *__restrict__ rec0, const JdRec *__restrict__ rec1,
                                                            const u32 *__restrict__ lane_part, u32 *__restrict__ lane_first,
                                                            int last_pass, const int *__restrict__ meta) {
  __shared__ u32 wsum[4];
  if (!settled(meta, last_pass)) return;
  const JdRec *rec = final_rec(rec0, rec1, meta);
  const u32 subs = (u32)meta[JD_M_SUBS];
  const u32 g0 = blockIdx.x * (u32)JD_LANES_PER_PART + threadIdx.x * (u32)LANES_PER_THREAD;
  u32 n[LANES_PER_THREAD], sum = 0;
#pragma unroll
  for (int j = 0; j < LANES_PER_THREAD; ++j) n[j] = g0 + j < subs ? rec[g0 + j].nblk : 0u, sum += n[j];
  u32 total;
  u32 at = lane_part[blockIdx.x] + block_excl_scan(sum, wsum, &total);
#pragma unroll
  for (int j = 0; j < LANES_PER_THREAD; ++j)
    if (g0 + j <= subs) lane_first[g0 + j] = at, at += n[j];            // (entry `subs` is the total)
}

// a thread per interval: its lanes' blocks must come to its MCUs x blocks per MCU
__global__ __launch_bounds__(256) void jd_check_kernel(JdParams p, const u32 *__restrict__ sub_first, const u32 *__restrict__ lane_first,
                                                       int last_pass, int *__restrict__ meta) {
  if (!settled(meta, last_pass)) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= p.n_iv) return;
  const u32 subs = (u32)meta[JD_M_SUBS];
  const u32 a = min(sub_first[k], subs), b = min(sub_first[k + 1], subs);
  const u32 blocks = lane_first[b] - lane_first[a];
  if (blocks != (u32)jd_interval_mcus(&p, k) * (u32)p.bpm) atomicOr(meta + JD_M_ERROR, JD_E_BLOCKS);
}

__global__ __launch_bounds__(256) void jd_write_kernel(JdParams p, const JdPlan *__restrict__ plan, const u32 *__restrict__ words,
                                                       const u32 *__restrict__ iv_start, const u32 *__restrict__ sub_first,
                                                       const JdRec *__restrict__ rec0, const JdRec *__restrict__ rec1,
                                                       const u32 *__restrict__ lane_first, int16_t *__restrict__ coef, int last_pass,
                                                       const int *__restrict__ meta) {
  __shared__ JdHuff huff[4];
  if (!settled(meta, last_pass)) return;
  const JdRec *rec = final_rec(rec0, rec1, meta);
  const u32 subs = (u32)meta[JD_M_SUBS];
  if (blockIdx.x * 256u >= subs) return;
  load_huff(huff, plan);
  const u32 g = blockIdx.x * 256u + threadIdx.x;
  if (g >= subs) return;
  const LaneSpan s = lane_span(iv_start, sub_first, p.n_iv, (u32)meta[JD_M_CLEAN], g);
  const JdRec r = rec[g];
  const uint64_t nominal = (uint64_t)s.bit0 + ((uint64_t)s.j + 1) * (u32)p.subseq_bits;
  const u32 sub_end = nominal < s.end_bits ? (u32)nominal : s.end_bits;
  const u32 base = (u32)s.k * (u32)p.restart * (u32)p.bpm;
  const u32 first = base + (lane_first[g] - lane_first[s.first_sub]);
  const u32 block_end = base + (u32)jd_interval_mcus(&p, s.k) * (u32)p.bpm;
  JdLane ln;
  ln.pos = min(r.in_pos, s.end_bits), ln.blk = (int)min(r.in_st >> 8, (u32)p.bpm - 1), ln.zz = (int)min(r.in_st & 255u, 63u), ln.nblk = 0;
  jd_lane_run(words, s.end_bits, sub_end, huff, &p, &ln, coef, first, block_end);
}

// DC differences -> DC values.  A thread per MCU, a workgroup per 256 MCUs.  apply == 0: the workgroup's summary to carry[chunk]
// = {sum of each component's differences behind the last interval start of the chunk (or in all of it), whether it holds a
// start}.  apply == 1: carry[chunk] holds the predictors that come into the chunk (jd_dc_carry_kernel); the values are written.
__global__ __launch_bounds__(256) void jd_dc_kernel(JdParams p, int16_t *__restrict__ coef, int *__restrict__ carry, int apply,
                                                    int last_pass, int *__restrict__ meta) {
  __shared__ int sum[2][3][256];
  __shared__ int flag[2][256];
  if (!settled(meta, last_pass)) return;
  const int t = threadIdx.x, m = blockIdx.x * 256 + t;
  int s[3] = {0, 0, 0};
  const bool live = m < p.total_mcus;
  if (live)
    for (int b = 0; b < p.bpm; ++b) s[p.blk_comp[b]] += coef[((size_t)m * p.bpm + b) * 64];
  int cur = 0;
  for (int c = 0; c < 3; ++c) sum[0][c][t] = s[c];
  flag[0][t] = live && m % p.restart == 0;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                                  // segmented inclusive scan (Hillis-Steele)
    const int nxt = cur ^ 1;
    const bool take = t >= o && !flag[cur][t];
    for (int c = 0; c < 3; ++c) sum[nxt][c][t] = sum[cur][c][t] + (take ? sum[cur][c][t - o] : 0);
    flag[nxt][t] = flag[cur][t] | (t >= o ? flag[cur][t - o] : 0);
    __syncthreads();
    cur = nxt;
  }
  if (!apply) {
    if (t == 255) {
      for (int c = 0; c < 3; ++c) carry[blockIdx.x * 4 + c] = sum[cur][c][255];
      carry[blockIdx.x * 4 + 3] = flag[cur][255];
    }
    return;
  }
  if (live) {
    int pred[3];
    for (int c = 0; c < 3; ++c) pred[c] = sum[cur][c][t] - s[c] + (flag[cur][t] ? 0 : carry[blockIdx.x * 4 + c]);
    for (int b = 0; b < p.bpm; ++b) {
      const size_t at = ((size_t)m * p.bpm + b) * 64;
      const int c = p.blk_comp[b];
      pred[c] += coef[at];
      coef[at] = (int16_t)max(-32768, min(32767, pred[c]));
    }
  }
  if (blockIdx.x == 0 && t == 0) meta[JD_M_COEF_DONE] = 1;
}

// one thread: the predictors that come into every chunk of 256 MCUs, in place of the chunks' summaries
__global__ void jd_dc_carry_kernel(int *__restrict__ carry, int chunks, int last_pass, const int *__restrict__ meta) {
  if (!settled(meta, last_pass)) return;
  int run[3] = {0, 0, 0};
  for (int ch = 0; ch < chunks; ++ch)
    for (int c = 0; c < 3; ++c) {
      const int tail = carry[ch * 4 + c];
      carry[ch * 4 + c] = run[c];
      run[c] = carry[ch * 4 + 3] ? tail : run[c] + tail;
    }
}

__global__ __launch_bounds__(256) void jd_idct_kernel(JdParams p, const JdPlan *__restrict__ plan, const int16_t *__restrict__ coef,
                                                      u8 *__restrict__ planes, int luma_w, int luma_h, int chroma_w, int chroma_h,
                                                      const int *__restrict__ meta) {
  if (meta[JD_M_ERROR] || !meta[JD_M_COEF_DONE]) return;
  const int64_t blk = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blk >= (int64_t)p.total_mcus * p.bpm) return;
  const int m = (int)(blk / p.bpm), b = (int)(blk % p.bpm), c = p.blk_comp[b];
  const int mr = m / p.mcu_cols, mc = m % p.mcu_cols;
  u8 *dst;
  int pitch;
  if (c == 0) {
    pitch = luma_w;
    dst = planes + (size_t)(mr * p.vs + b / p.hs) * 8 * pitch + (size_t)(mc * p.hs + b % p.hs) * 8;
  } else {
    pitch = chroma_w;
    dst = planes + (size_t)luma_w * luma_h + (size_t)(c - 1) * chroma_w * chroma_h + (size_t)mr * 8 * pitch + (size_t)mc * 8;
  }
  const u8 *q = plan->t.quant[p.comp_tq[c]];
  const int16_t *src = coef + blk * 64;
  static constexpr u8 JD_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  int32_t in[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) in[JD_ZIGZAG[k]] = (int32_t)src[k] * (int32_t)q[JD_ZIGZAG[k]];
  jd_idct_block(in, dst, pitch);
}

__global__ __launch_bounds__(256) void jd_rgb_kernel(JdParams p, const u8 *__restrict__ planes, int luma_w, int luma_h, int chroma_w,
                                                     int chroma_h, u8 *__restrict__ rgb, const int *__restrict__ meta) {
  if (meta[JD_M_ERROR] || !meta[JD_M_COEF_DONE]) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.w * p.h) return;
  const int y = (int)(i / p.w), x = (int)(i % p.w);
  const int lum = planes[(size_t)y * luma_w + x];
  u8 *out = rgb + i * 3;
  if (p.ncomp == 1) {
    out[0] = out[1] = out[2] = (u8)lum;
    return;
  }
  const u8 *cbp = planes + (size_t)luma_w * luma_h, *crp = cbp + (size_t)chroma_w * chroma_h;
  const int cw = (p.w + p.hs - 1) / p.hs, ch = (p.h + p.vs - 1) / p.vs;
  u8 px[3];
  jd_ycc_rgb(lum, jd_chroma_at(cbp, chroma_w, cw, ch, p.hs, p.vs, x, y), jd_chroma_at(crp, chroma_w, cw, ch, p.hs, p.vs, x, y), px);
  out[0] = px[0], out[1] = px[1], out[2] = px[2];
}

bool plan_ok(const void *plan) { return plan && ((const JdPlan *)plan)->p.magic == JD_MAGIC; }

}  // namespace

extern "C" size_t sp_jpeg_decode_plan_bytes(void) { return (sizeof(JdPlan) + 255) & ~(size_t)255; }

extern "C" int sp_jpeg_decode_plan(const int32_t *fields, const uint8_t *quant4x64, int have_quant, const uint8_t *bits4x16,
                                   const uint8_t *vals4x256, int have_huff, void *plan) {
  SP_REQUIRE(fields && quant4x64 && bits4x16 && vals4x256 && plan, "sp_jpeg_decode_plan: null pointer");
  JdPlan pl = {};
  const char *why = "";
  if (jd_make_plan(fields, quant4x64, have_quant, bits4x16, vals4x256, have_huff, &pl, &why) != 0) {
    sp_set_error("sp_jpeg_decode_plan: %s", why);
    return SP_EINVAL;
  }
  memset(plan, 0, sp_jpeg_decode_plan_bytes());
  memcpy(plan, &pl, sizeof(pl));
  return SP_OK;
}

extern "C" size_t sp_jpeg_decode_ws_bytes(const void *plan) {
  if (!plan_ok(plan)) return 0;
  JdLayout L;
  jd_layout(&((const JdPlan *)plan)->p, &L);
  return L.total;
}

extern "C" size_t sp_jpeg_decode_coef_bytes(const void *plan) {
  if (!plan_ok(plan)) return 0;
  const JdParams &p = ((const JdPlan *)plan)->p;
  return (size_t)p.total_mcus * p.bpm * 64 * sizeof(int16_t);
}

#define JD_COMMON(name)                                                                                                       \
  SP_REQUIRE(plan && plan_dev && ws, name ": null pointer");                                                                  \
  SP_REQUIRE(plan_ok(plan), name ": plan was not made by sp_jpeg_decode_plan");                                               \
  const JdParams &p = ((const JdPlan *)plan)->p;                                                                              \
  JdLayout L;                                                                                                                 \
  jd_layout(&p, &L);                                                                                                          \
  SP_REQUIRE(ws_bytes >= L.total, name ": ws holds %zu bytes, needs %zu (sp_jpeg_decode_ws_bytes)", ws_bytes, L.total);       \
  SP_REQUIRE((uintptr_t)ws % 16 == 0 && (uintptr_t)plan_dev % 16 == 0, name ": ws and plan_dev must be 16-byte aligned");     \
  hipStream_t s = (hipStream_t)stream;                                                                                        \
  char *base = (char *)ws;                                                                                                    \
  int *meta = (int *)(base + L.meta);                                                                                         \
  (void)s, (void)base, (void)meta

extern "C" int sp_jpeg_decode_split(const void *plan, const void *plan_dev, const void *segment, void *ws, size_t ws_bytes,
                                    void *stream) {
  JD_COMMON("sp_jpeg_decode_split");
  SP_REQUIRE(segment, "sp_jpeg_decode_split: null pointer");
  SP_CLEAR_STALE_ERROR();
  hipMemsetAsync(meta, 0, JD_M_WORDS * 4, s);
  u32 *blk_keep = (u32 *)(base + L.blk_keep), *blk_mark = (u32 *)(base + L.blk_mark);
  u32 *iv_start = (u32 *)(base + L.iv_start);
  hipLaunchKernelGGL(jd_count_kernel, dim3(L.byte_blocks), dim3(256), 0, s, (const u8 *)segment, p.seg_len, blk_keep, blk_mark, meta);
  hipLaunchKernelGGL(jd_scan_bytes_kernel, dim3(1), dim3(256), 0, s, blk_keep, blk_mark, L.byte_blocks, p.n_iv, iv_start, meta);
  hipLaunchKernelGGL(jd_compact_kernel, dim3(L.byte_blocks), dim3(256), 0, s, (const u8 *)segment, p.seg_len, blk_keep, blk_mark,
                     p.n_iv, (u8 *)(base + L.clean), iv_start, meta);
  hipLaunchKernelGGL(jd_intervals_kernel, dim3(1), dim3(256), 0, s, iv_start, p.n_iv, p.subseq_bits, p.max_sub,
                     (u32 *)(base + L.sub_first), meta);
  SP_CHECK_LAUNCH("sp_jpeg_decode_split");
  return SP_OK;
}

extern "C" int sp_jpeg_decode_sync(const void *plan, const void *plan_dev, void *ws, size_t ws_bytes, int first_pass, int passes,
                                   void *stream) {
  JD_COMMON("sp_jpeg_decode_sync");
  SP_REQUIRE(first_pass >= 0 && passes >= 1 && passes <= 4096 && first_pass <= 0x7fffffff - passes,
             "sp_jpeg_decode_sync: first_pass must be >= 0 and passes 1..4096 (first_pass=%d, passes=%d)", first_pass, passes);
  SP_CLEAR_STALE_ERROR();
  JdRec *rec[2] = {(JdRec *)(base + L.rec0), (JdRec *)(base + L.rec1)};
  const unsigned grid = (unsigned)((p.max_sub + 255) / 256);
  for (int q = first_pass; q < first_pass + passes; ++q)
    hipLaunchKernelGGL(jd_pass_kernel, dim3(grid), dim3(256), 0, s, p, (const JdPlan *)plan_dev, (const u32 *)(base + L.clean),
                       (const u32 *)(base + L.iv_start), (const u32 *)(base + L.sub_first), (const JdRec *)rec[(q + 1) & 1],
                       rec[q & 1], q, meta);
  SP_CHECK_LAUNCH("sp_jpeg_decode_sync");
  return SP_OK;
}

extern "C" int sp_jpeg_decode_coefficients(const void *plan, const void *plan_dev, void *ws, size_t ws_bytes, int last_pass,
                                           void *coef, void *stream) {
  JD_COMMON("sp_jpeg_decode_coefficients");
  SP_REQUIRE(coef && (uintptr_t)coef % 2 == 0, "sp_jpeg_decode_coefficients: coef must be a 2-byte aligned pointer");
  SP_REQUIRE(last_pass >= 0, "sp_jpeg_decode_coefficients: last_pass must be >= 0 (got %d)", last_pass);
  SP_CLEAR_STALE_ERROR();
  const JdRec *rec0 = (const JdRec *)(base + L.rec0), *rec1 = (const JdRec *)(base + L.rec1);
  u32 *lane_part = (u32 *)(base + L.lane_part), *lane_first = (u32 *)(base + L.lane_first);
  const u32 *sub_first = (const u32 *)(base + L.sub_first);
  int *carry = (int *)(base + L.dc_carry);
  hipMemsetAsync(coef, 0, sp_jpeg_decode_coef_bytes(plan), s);
  hipLaunchKernelGGL(jd_lane_sum_kernel, dim3(L.lane_parts), dim3(256), 0, s, rec0, rec1, lane_part, last_pass, meta);
  hipLaunchKernelGGL(jd_scan_small_kernel, dim3(1), dim3(256), 0, s, lane_part, L.lane_parts, last_pass, (const int *)meta);
  hipLaunchKernelGGL(jd_lane_first_kernel, dim3(L.lane_parts), dim3(256), 0, s, rec0, rec1, (const u32 *)lane_part, lane_first, last_pass,
                     (const int *)meta);
  hipLaunchKernelGGL(jd_check_kernel, dim3((p.n_iv + 255) / 256), dim3(256), 0, s, p, sub_first, (const u32 *)lane_first, last_pass, meta);
  hipLaunchKernelGGL(jd_write_kernel, dim3((p.max_sub + 255) / 256), dim3(256), 0, s, p, (const JdPlan *)plan_dev,
                     (const u32 *)(base + L.clean), (const u32 *)(base + L.iv_start), sub_first, rec0, rec1, (const u32 *)lane_first,
                     (int16_t *)coef, last_pass, (const int *)meta);
  hipLaunchKernelGGL(jd_dc_kernel, dim3(L.dc_chunks), dim3(256), 0, s, p, (int16_t *)coef, carry, 0, last_pass, meta);
  hipLaunchKernelGGL(jd_dc_carry_kernel, dim3(1), dim3(1), 0, s, carry, L.dc_chunks, last_pass, (const int *)meta);
  hipLaunchKernelGGL(jd_dc_kernel, dim3(L.dc_chunks), dim3(256), 0, s, p, (int16_t *)coef, carry, 1, last_pass, meta);
  SP_CHECK_LAUNCH("sp_jpeg_decode_coefficients");
  return SP_OK;
}

extern "C" int sp_jpeg_decode_pixels(const void *plan, const void *plan_dev, void *ws, size_t ws_bytes, const void *coef, void *rgb,
                                     void *stream) {
  JD_COMMON("sp_jpeg_decode_pixels");
  SP_REQUIRE(coef && rgb && (uintptr_t)coef % 2 == 0, "sp_jpeg_decode_pixels: coef (2-byte aligned) and rgb must not be null");
  SP_CLEAR_STALE_ERROR();
  u8 *planes = (u8 *)(base + L.planes);
  const int64_t blocks = (int64_t)p.total_mcus * p.bpm, pixels = (int64_t)p.w * p.h;
  hipLaunchKernelGGL(jd_idct_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, p, (const JdPlan *)plan_dev,
                     (const int16_t *)coef, planes, L.luma_w, L.luma_h, L.chroma_w, L.chroma_h, (const int *)meta);
  hipLaunchKernelGGL(jd_rgb_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, p, (const u8 *)planes, L.luma_w, L.luma_h,
                     L.chroma_w, L.chroma_h, (u8 *)rgb, (const int *)meta);
  SP_CHECK_LAUNCH("sp_jpeg_decode_pixels");
  return SP_OK;
}
