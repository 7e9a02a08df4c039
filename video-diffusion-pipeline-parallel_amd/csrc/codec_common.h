// What the image codecs (jpeg.hip, gif.hip, png.hip, webp.hip; crc32.hip for the typedefs) say in the same words: the sums
// over a workgroup of 256, the LSB-first bit writer and reader of the staging words, and the prefix-code builder of deflate
// and VP8L.  Everything here is a template or static / __forceinline__: nothing is exported, and every file keeps its tables,
// its Strip and its format's rules.  The byte-exact models (tests/{png,webp}_model.py) restate the builder's tie rules.
#pragma once
#include "common.h"

typedef unsigned char u8;
typedef unsigned short u16;
typedef unsigned int u32;
typedef unsigned long long u64;

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// what a residual byte costs a filter or predictor choice: its distance from 0 mod 256
__device__ __forceinline__ u32 byte_cost(int v) {
  v &= 255;
  return (u32)min(v, 256 - v);
}

// ---------------------------------------------------------------------------------------------- sums
__device__ __forceinline__ int wave_inclusive_sum(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// exclusive sum of v over a workgroup of 256; total in `all`.  wave_val: 4 words of LDS, free again after the next barrier.
__device__ __forceinline__ int block_exclusive_sum(int (&wave_val)[4], int v, int &all) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int incl = wave_inclusive_sum(v);
  __syncthreads();
  if (lane == 63) wave_val[wv] = incl;
  __syncthreads();
  int before = 0;
  for (int i = 0; i < wv; ++i) before += wave_val[i];
  all = wave_val[0] + wave_val[1] + wave_val[2] + wave_val[3];
  return before + incl - v;
}

// The same over value(0 .. count), 256 entries a round, the total so far carried from round to round: store(k, start + the
// sum before k) for every k, by the thread that took value(k).  -> start + the sum of all, to every thread.
template <class Value, class Store>
__device__ __forceinline__ int carried_exclusive_sum(int (&wave_val)[4], int count, int start, Value value, Store store) {
  int running = start;
  for (int k0 = 0; k0 < count; k0 += 256) {
    const int k = k0 + (int)threadIdx.x;
    const int v = k < count ? value(k) : 0;
    int all;
    const int before = running + block_exclusive_sum(wave_val, v, all);
    if (k < count) store(k, before);
    running += all;
  }
  return running;
}

// ---------------------------------------------------------------------------------------------- bits, LSB first
// the 8 bits from bit p of words on
__device__ __forceinline__ u32 bits8(const u32 *__restrict__ words, int p) {
  const int wd = p >> 5, sh = p & 31;
  u32 v = words[wd] >> sh;
  if (sh > 24) v |= words[wd + 1] << (32 - sh);
  return v & 255u;
}

// one thread: `width` <= 32 bits of value ORed into the zeroed words at bit `at`, which moves on
__device__ __forceinline__ void put_bits(u32 *words, int &at, u32 value, int width) {
  if (width == 0) return;
  const int a = at;
  words[a >> 5] |= value << (a & 31);
  if ((a & 31) + width > 32) words[(a >> 5) + 1] |= value >> (32 - (a & 31));
  at = a + width;
}

// ---------------------------------------------------------------------------------------------- code construction
// NSYM: the including file's largest alphabet (286 for deflate, 280 for VP8L), so that the kernel's LDS is what it needs
template <int NSYM>
struct HuffBuilder {
  u32 cnt[NSYM];
  u16 order[NSYM];                      // sorted place -> symbol
  u32 weight[2 * NSYM];                 // the leaves in sorted order, then the joined nodes in order of their making
  u16 parent[2 * NSYM];
  u16 depth[2 * NSYM];
  u32 next_code[17];
  int leaves, deepest;
};

// Code lengths of B.cnt[0 .. nsym) into len[0 .. nsym), by every thread of the workgroup of 256.  B.cnt is changed.  A rank
// sort by (count, symbol) by all threads, the two-queue merge and the depths by one thread, the halving loop around both.
template <int NSYM>
__device__ void build_lengths(HuffBuilder<NSYM> &B, int nsym, int limit, u8 *len) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid == 0) {
    int used = 0;
    for (int s = 0; s < nsym; ++s) used += B.cnt[s] != 0;
    for (int s = 0; used < 2 && s < nsym; ++s)
      if (!B.cnt[s]) { B.cnt[s] = 1; ++used; }
  }
  // A count is 1 after at most 25 halvings, and with all counts at 1 the tree over 286 symbols is 9 deep and over 19 symbols
  // 5 deep, below the limits of 15 and 7: the bound is never why the loop ends.
  for (int round = 0; round < 32; ++round) {
    __syncthreads();
    for (int s = tid; s < nsym; s += 256) {
      const u32 c = B.cnt[s];
      len[s] = 0;
      if (c) {
        int r = 0;
        for (int t = 0; t < nsym; ++t) {
          const u32 ct = B.cnt[t];
          r += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1 : 0;
        }
        B.order[r] = (u16)s;
        B.weight[r] = c;
      }
    }
    __syncthreads();
    if (tid == 0) {
      int L = 0;
      for (int s = 0; s < nsym; ++s) L += B.cnt[s] != 0;
      int i = 0, j = 0;                                     // the next leaf, the next joined node
      for (int m = 0; m < L - 1; ++m) {
        int pick[2];
        for (int k = 0; k < 2; ++k) {                       // (equal weights: the leaf, which is older)
          if (i < L && (j >= m || B.weight[i] <= B.weight[L + j])) pick[k] = i++;
          else pick[k] = L + j++;
        }
        B.weight[L + m] = B.weight[pick[0]] + B.weight[pick[1]];
        B.parent[pick[0]] = (u16)(L + m);
        B.parent[pick[1]] = (u16)(L + m);
      }
      B.depth[2 * L - 2] = 0;
      for (int node = 2 * L - 3; node >= L; --node) B.depth[node] = B.depth[B.parent[node]] + 1;
      B.leaves = L;
      B.deepest = 0;
    }
    __syncthreads();
    const int L = B.leaves;
    int deepest = 0;
    for (int i = tid; i < L; i += 256) {
      const int d = B.depth[B.parent[i]] + 1;
      len[B.order[i]] = (u8)min(d, 255);
      deepest = max(deepest, d);
    }
    if (deepest) atomicMax(&B.deepest, deepest);
    __syncthreads();
    if (B.deepest <= limit) break;
    for (int s = tid; s < nsym; s += 256) {
      const u32 c = B.cnt[s];
      B.cnt[s] = c ? (c + 1) >> 1 : 0;
    }
  }
  __syncthreads();
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first packing
template <int NSYM>
__device__ void canonical_codes(HuffBuilder<NSYM> &B, int nsym, const u8 *len, u16 *code) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid == 0) {
    u32 count[17];
    for (int b = 0; b < 17; ++b) count[b] = 0;
    for (int s = 0; s < nsym; ++s) ++count[len[s]];
    count[0] = 0;
    u32 c = 0;
    B.next_code[0] = 0;
    for (int b = 1; b < 17; ++b) {
      c = (c + count[b - 1]) << 1;
      B.next_code[b] = c;
    }
  }
  __syncthreads();
  for (int s = tid; s < nsym; s += 256) {
    const int n = len[s];
    u32 c = 0;
    if (n) {
      c = B.next_code[n];
      for (int t = 0; t < s; ++t) c += len[t] == n ? 1 : 0;
      c = __brev(c) >> (32 - n);
    }
    code[s] = (u16)c;
  }
  __syncthreads();
}

// One thread: zlib's scan of len[0 .. n) appended to seq[nseq ..) as symbol | extra value << 5, counts into cnt.  In VP8L a 16
// repeats "the last non-zero length"; a 16 here always follows its own length, so that is the same value as deflate's "the
// previous length".
static __device__ void run_length_form(u16 *seq, int &nseq, u32 *cnt, const u8 *len, int n) {
  int prev = -1, count = 0, nxt = len[0];
  int max_count = nxt == 0 ? 138 : 7, min_count = nxt == 0 ? 3 : 4;
  auto emit = [&](int sym, int value) {
    seq[nseq++] = (u16)(sym | (value << 5));
    ++cnt[sym];
  };
  for (int i = 0; i < n; ++i) {
    const int cur = nxt;
    nxt = i + 1 < n ? len[i + 1] : -1;
    if (++count < max_count && cur == nxt) continue;
    if (count < min_count) {
      for (int k = 0; k < count; ++k) emit(cur, 0);
    } else if (cur != 0) {
      if (cur != prev) { emit(cur, 0); --count; }
      emit(16, count - 3);
    } else if (count <= 10) {
      emit(17, count - 3);
    } else {
      emit(18, count - 11);
    }
    count = 0;
    prev = cur;
    if (nxt == 0) { max_count = 138; min_count = 3; }
    else if (cur == nxt) { max_count = 6; min_count = 3; }
    else { max_count = 7; min_count = 4; }
  }
}
