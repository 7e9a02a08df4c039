// Animated GIF of uint8 frames that are already in device memory: the other file of the reference's demo
// (save_gif, scripts/generate_video_demo.py:212-222 there, leaves it to imageio / Pillow).  The library makes,
// per frame, a 256-entry palette, the index of every pixel, and the complete image data of a GIF image block; the file
// around them is host work (models/image_io.py write_gif).
//
// Quantiser (integer arithmetic throughout: include/svdpipe.h fixes the rules, tests/gif_model.py restates them):
//   gif_hist_kernel  : four pixels per thread; count and the three channel sums of the 32^3 bins in two 64-bit words per bin
//                      (count << 32 | R sum, G sum << 32 | B sum: no field can carry while h*w <= 2^24), one atomic add per
//                      word and run of equal bins.
//   gif_svt_kernel   : per (frame, quantity) one workgroup turns the histogram into a summed-volume table of 33^3 words
//                      (S[x][y][z] = everything below x, y, z), three passes of 1024 line scans; the sum over any box is eight
//                      reads, in 32-bit arithmetic that wraps and comes out right because the true value fits.
//   gif_split_kernel : one workgroup per frame does the up to 255 splits.  Box limits and counts live in LDS; a step is an
//                      arg-max over the boxes, 32 lanes taking the running plane counts of the chosen box (one box sum each)
//                      and a ballot finding the cut, then 192 lanes shrinking the two parts (a lane per part, axis and plane:
//                      is that slab occupied?  ballot, first and last bit).  Then the palette: four box sums per entry.
//   gif_table_kernel : bin -> index: a thread per bin runs over the entries in use (palette in LDS).
//   gif_map_kernel   : four pixels per thread through that table.
// LZW, strip-parallel:
//   gif_lzw_kernel   : one wave per strip.  The dictionary is an open-addressed table of 8192 words in LDS (key = prefix code
//                      and pixel, 20 bits, over the 12-bit code; 0 = free, which no entry equals as codes start at 258).  The
//                      chain is serial, so all 64 lanes walk it in step on the same values (every LDS read is a broadcast, no
//                      branch diverges); what the wave shares out is the table clear and the fetch of the next 1024 pixels
//                      into LDS.  Lane 0 stores the packed codes, 32 bits at a time, into the strip's staging slot.
//   gif_scan_kernel  : per frame the exclusive sum of the strips' bit counts, the byte count, the 08 in front and the
//                      terminator behind.
//   gif_place_kernel : one workgroup per strip writes the data bytes whose first bit lies in the strip (a byte that runs over
//                      the strip's end takes its high bits from the head of the next strip), each at j + 2 + j / 255, and the
//                      length byte in front of every 255th.
// Nothing here is tuned beyond its layout; profiles/gif_timing.txt has what it costs.
#include "codec_common.h"

namespace {

constexpr int BINS = 32 * 32 * 32;
constexpr int SV = 33, SVN = SV * SV * SV;
constexpr size_t HIST_BYTES = 2 * (size_t)BINS * sizeof(u64);
constexpr size_t SVT_BYTES = ((4 * (size_t)SVN * sizeof(u32) + 255) / 256) * 256;
constexpr size_t TABLE_BYTES = BINS;
constexpr int MAX_PIXELS = 1 << 24;

constexpr int LZW_CLEAR = 256, LZW_EOI = 257, LZW_FIRST = 258, LZW_END = 4096;
constexpr int LZW_SLOTS = 8192, LZW_CHUNK = 1024;
constexpr int LZW_ENTRIES = LZW_END - LZW_FIRST;          // 3838 codes fill the table

bool gif_dims_ok(int h, int w) { return h > 0 && w > 0 && h <= 65535 && w <= 65535 && (int64_t)h * w <= MAX_PIXELS; }

// ---------------------------------------------------------------------------------------------- pixels, four at a time
// pixels p0 .. p0+cnt-1 of the flat (n*h*w, 3) array
__device__ __forceinline__ void load_pixels(const u8 *__restrict__ frames, int64_t p0, int cnt, bool aligned, u8 (&px)[12]) {
  const u8 *p = frames + p0 * 3;
  if (aligned && cnt == 4) {
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
    for (int e = 0; e < 12; ++e) px[e] = e < 3 * cnt ? p[e] : (u8)0;
  }
}

__device__ __forceinline__ int bin_of(int r, int g, int b) { return ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3); }

__global__ __launch_bounds__(256) void gif_hist_kernel(const u8 *__restrict__ frames, int64_t total, int hw, int aligned,
                                                       u64 *__restrict__ hist) {
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= total) return;
  const int cnt = (int)min((int64_t)4, total - p0);
  u8 px[12];
  load_pixels(frames, p0, cnt, aligned != 0, px);
  int64_t f = p0 / hw;
  int at = (int)(p0 - f * hw);
  u64 a0 = 0, a1 = 0;
  int64_t slot = -1;
  for (int e = 0; e < cnt; ++e) {
    const int r = px[3 * e], g = px[3 * e + 1], b = px[3 * e + 2];
    const int64_t s = f * (2 * BINS) + bin_of(r, g, b);
    if (s != slot) {
      if (slot >= 0) { atomicAdd(&hist[slot], a0); atomicAdd(&hist[slot + BINS], a1); }
      slot = s; a0 = 0; a1 = 0;
    }
    a0 += (1ull << 32) | (u64)r;
    a1 += ((u64)g << 32) | (u64)b;
    if (++at == hw) { at = 0; ++f; }
  }
  atomicAdd(&hist[slot], a0);
  atomicAdd(&hist[slot + BINS], a1);
}

// quantity q of a bin: 0 the count, 1 .. 3 the sums of R, G, B
__device__ __forceinline__ u32 hist_field(const u64 *__restrict__ hist, int bin, int q) {
  const u64 v = hist[(q >> 1) * BINS + bin];
  return (q & 1) ? (u32)v : (u32)(v >> 32);
}

// grid: n * 4 workgroups of 1024
__global__ __launch_bounds__(1024) void gif_svt_kernel(const u64 *__restrict__ hist_all, u32 *__restrict__ svt_all, int64_t svt_words) {
  const int tid = threadIdx.x, a = tid >> 5, b = tid & 31;
  const int64_t f = blockIdx.x >> 2;
  const int q = blockIdx.x & 3;
  const u64 *hist = hist_all + f * (2 * BINS);
  u32 *S = svt_all + f * svt_words + (int64_t)q * SVN;
  {  // along z: line (x, y) = (a, b)
    u32 run = 0;
    u32 *line = S + ((a + 1) * SV + (b + 1)) * SV;
    line[0] = 0;
    for (int z = 0; z < 32; ++z) {
      run += hist_field(hist, (a << 10) | (b << 5) | z, q);
      line[z + 1] = run;
    }
  }
  for (int i = tid; i < SV * SV; i += 1024) {
    S[i] = 0;                                              // the face x = 0
    S[(i / SV) * SV * SV + (i % SV)] = 0;                  // the face y = 0
  }
  __syncthreads();
  {  // along y: line (x, z) = (a + 1, b + 1)
    u32 run = 0;
    for (int y = 1; y <= 32; ++y) {
      u32 *p = S + ((a + 1) * SV + y) * SV + b + 1;
      run += *p;
      *p = run;
    }
  }
  __syncthreads();
  {  // along x: line (y, z) = (a + 1, b + 1)
    u32 run = 0;
    for (int x = 1; x <= 32; ++x) {
      u32 *p = S + (x * SV + a + 1) * SV + b + 1;
      run += *p;
      *p = run;
    }
  }
}

struct Box { int lo[3], hi[3]; };   // inclusive

__device__ __forceinline__ u32 box_sum(const u32 *__restrict__ S, const Box &bx) {
  const int x0 = bx.lo[0], y0 = bx.lo[1], z0 = bx.lo[2], x1 = bx.hi[0] + 1, y1 = bx.hi[1] + 1, z1 = bx.hi[2] + 1;
  auto at = [&](int x, int y, int z) { return S[(x * SV + y) * SV + z]; };
  return at(x1, y1, z1) - at(x0, y1, z1) - at(x1, y0, z1) - at(x1, y1, z0) + at(x0, y0, z1) + at(x0, y1, z0) + at(x1, y0, z0) -
         at(x0, y0, z0);
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u32 hi = __shfl_xor((u32)(v >> 32), o, 64), lo = __shfl_xor((u32)v, o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    v = other > v ? other : v;
  }
  return v;
}

// grid: n workgroups of 256
__global__ __launch_bounds__(256) void gif_split_kernel(const u32 *__restrict__ svt_all, int64_t svt_words, u8 *__restrict__ palette,
                                                        int *__restrict__ nbox_out) {
  __shared__ int lo[3][256], hi[3][256];
  __shared__ u32 cnt[256];
  __shared__ u64 red[4];
  __shared__ Box part[2];              // the two parts of a split before they are shrunk
  __shared__ int part_on[2];
  __shared__ u32 part_cnt[2];
  __shared__ int new_lo[2][3], new_hi[2][3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t f = blockIdx.x;
  const u32 *S = svt_all + f * svt_words;            // quantity 0: the counts

  // threads 0..191: part k, axis ax, plane p -- is the slab p of part k occupied?  first and last set bit are the shrunk limits
  auto shrink_parts = [&]() {
    const int k = tid / 96, ax = (tid % 96) >> 5, p = tid & 31;
    bool occupied = false;
    if (tid < 192 && part_on[k]) {
      Box bx = part[k];
      if (p >= bx.lo[ax] && p <= bx.hi[ax]) {
        bx.lo[ax] = p; bx.hi[ax] = p;
        occupied = box_sum(S, bx) != 0;
      }
    }
    const u64 mask = __ballot(occupied);
    const u32 half = (tid & 32) ? (u32)(mask >> 32) : (u32)mask;
    if (tid < 192 && part_on[k] && p == 0) {
      new_lo[k][ax] = __builtin_ctz(half);
      new_hi[k][ax] = 31 - __builtin_clz(half);
    }
  };

  if (tid == 0) {
    for (int ax = 0; ax < 3; ++ax) { part[0].lo[ax] = 0; part[0].hi[ax] = 31; }
    part_on[0] = 1; part_on[1] = 0;
  }
  __syncthreads();
  shrink_parts();
  __syncthreads();
  if (tid < 3) { lo[tid][0] = new_lo[0][tid]; hi[tid][0] = new_hi[0][tid]; }
  if (tid == 0) { cnt[0] = S[SVN - 1]; part_on[1] = 1; }
  __syncthreads();

  int nb = 1;
  while (nb < 256) {
    // the box with the largest count * extent; the lowest index among equals
    u64 key = 0;
    if (tid < nb) {
      const int e = max(max(hi[0][tid] - lo[0][tid], hi[1][tid] - lo[1][tid]), hi[2][tid] - lo[2][tid]);
      if (e > 0) key = ((u64)cnt[tid] * (u64)e << 8) | (u64)(255 - tid);
    }
    key = wave_max_u64(key);
    if (lane == 0) red[tid >> 6] = key;
    __syncthreads();
    const u64 best = max(max(red[0], red[1]), max(red[2], red[3]));
    if (best == 0) break;                                  // (every thread reads the same four words)
    const int b = 255 - (int)(best & 255);
    if (tid < 64) {
      Box bx;
      for (int ax = 0; ax < 3; ++ax) { bx.lo[ax] = lo[ax][b]; bx.hi[ax] = hi[ax][b]; }
      const int e = max(max(bx.hi[0] - bx.lo[0], bx.hi[1] - bx.lo[1]), bx.hi[2] - bx.lo[2]);
      const int axis = bx.hi[0] - bx.lo[0] == e ? 0 : (bx.hi[1] - bx.lo[1] == e ? 1 : 2);
      const u32 pixels = cnt[b];
      u32 running = 0;
      if (lane <= e) {
        Box sub = bx;
        sub.hi[axis] = bx.lo[axis] + lane;
        running = box_sum(S, sub);
      }
      const u64 enough = __ballot(lane <= e && 2ull * running >= pixels);   // lane e always: its sum is the box's count
      const int c = min((int)__builtin_ctzll(enough), e - 1);
      const u32 lower = __shfl(running, c, 64);
      if (lane == 0) {
        part[0] = bx; part[1] = bx;
        part[0].hi[axis] = bx.lo[axis] + c;
        part[1].lo[axis] = bx.lo[axis] + c + 1;
        part_cnt[0] = lower; part_cnt[1] = pixels - lower;
      }
    }
    __syncthreads();
    shrink_parts();
    __syncthreads();
    if (tid < 3) {
      lo[tid][b] = new_lo[0][tid]; hi[tid][b] = new_hi[0][tid];
      lo[tid][nb] = new_lo[1][tid]; hi[tid][nb] = new_hi[1][tid];
    }
    if (tid == 0) { cnt[b] = part_cnt[0]; cnt[nb] = part_cnt[1]; }
    ++nb;
    __syncthreads();
  }
  // entry i: the rounded mean of box i
  u8 *pal = palette + f * 768 + tid * 3;
  if (tid < nb) {
    Box bx;
    for (int ax = 0; ax < 3; ++ax) { bx.lo[ax] = lo[ax][tid]; bx.hi[ax] = hi[ax][tid]; }
    const u64 c = cnt[tid];
    for (int ch = 0; ch < 3; ++ch) pal[ch] = (u8)((2ull * box_sum(S + (ch + 1) * SVN, bx) + c) / (2ull * c));
  } else {
    pal[0] = 0; pal[1] = 0; pal[2] = 0;
  }
  if (tid == 0) nbox_out[f] = nb;
}

// grid: n * 128 workgroups of 256, a thread per bin
__global__ __launch_bounds__(256) void gif_table_kernel(const u64 *__restrict__ hist_all, const u8 *__restrict__ palette,
                                                        const int *__restrict__ nbox, u8 *__restrict__ table_all) {
  __shared__ int pal[256 * 3];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x >> 7;
  const int bin = ((blockIdx.x & 127) << 8) | tid;
  const int used = nbox[f];
  for (int i = tid; i < 768; i += 256) pal[i] = palette[f * 768 + i];
  __syncthreads();
  const u64 *hist = hist_all + f * (2 * BINS);
  const u64 c = hist_field(hist, bin, 0);
  int best = 0;
  if (c) {
    const int r = (int)((2ull * hist_field(hist, bin, 1) + c) / (2ull * c)), g = (int)((2ull * hist_field(hist, bin, 2) + c) / (2ull * c)),
              b = (int)((2ull * hist_field(hist, bin, 3) + c) / (2ull * c));
    int best_d = 0x7fffffff;
    for (int i = 0; i < used; ++i) {
      const int dr = r - pal[3 * i], dg = g - pal[3 * i + 1], db = b - pal[3 * i + 2];
      const int d = dr * dr + dg * dg + db * db;
      if (d < best_d) { best_d = d; best = i; }
    }
  }
  table_all[f * BINS + bin] = (u8)best;
}

__global__ __launch_bounds__(256) void gif_map_kernel(const u8 *__restrict__ frames, int64_t total, int hw, int aligned,
                                                      int out_aligned, const u8 *__restrict__ table_all, u8 *__restrict__ indices) {
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= total) return;
  const int cnt = (int)min((int64_t)4, total - p0);
  u8 px[12];
  load_pixels(frames, p0, cnt, aligned != 0, px);
  int64_t f = p0 / hw;
  int at = (int)(p0 - f * hw);
  u8 idx[4] = {0, 0, 0, 0};
  for (int e = 0; e < cnt; ++e) {
    idx[e] = table_all[f * BINS + bin_of(px[3 * e], px[3 * e + 1], px[3 * e + 2])];
    if (++at == hw) { at = 0; ++f; }
  }
  if (out_aligned && cnt == 4) {
    *(u32 *)(indices + p0) = (u32)idx[0] | ((u32)idx[1] << 8) | ((u32)idx[2] << 16) | ((u32)idx[3] << 24);
  } else {
    for (int e = 0; e < cnt; ++e) indices[p0 + e] = idx[e];
  }
}

// ---------------------------------------------------------------------------------------------- LZW
// The bits one strip of `pixels` pixels can take: a code per pixel at most, 12 bits each; a CLEAR after every 3838 codes; the
// code that ends the strip; and the frame's opening CLEAR (9 bits) in the first strip's string.
__host__ __device__ inline int64_t strip_bits_bound(int64_t pixels) { return 9 + 12 * pixels + 12 * (pixels / LZW_ENTRIES) + 12; }
int64_t slot_bytes_of(int64_t pixels) { return ((strip_bits_bound(pixels) + 31) / 32 + 1) * 4; }   // whole words, one to spare

// grid: one 64-thread workgroup per (frame, strip)
__global__ __launch_bounds__(64) void gif_lzw_kernel(const u8 *__restrict__ indices, int h, int w, int strip_rows, int strips,
                                                     u8 *__restrict__ stage, int64_t slot_bytes, int *__restrict__ bits_out) {
  __shared__ u32 tab[LZW_SLOTS];
  __shared__ u8 pix[LZW_CHUNK];
  const int lane = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int s = (int)(bid % strips);
  const int64_t f = bid / strips;
  const int rows = min(strip_rows, h - s * strip_rows);
  const int pixels = rows * w;
  const u8 *src = indices + (f * h + (int64_t)s * strip_rows) * w;
  u32 *dst = (u32 *)(stage + bid * slot_bytes);

  auto clear = [&]() {
    __syncthreads();
    for (int i = lane; i < LZW_SLOTS; i += 64) tab[i] = 0;
    __syncthreads();
  };
  u64 acc = 0;
  int held = 0, word = 0, total = 0;
  auto put = [&](u32 code, int width) {
    acc |= (u64)code << held;
    held += width;
    total += width;
    if (held >= 32) {
      if (lane == 0) dst[word] = (u32)acc;
      ++word;
      acc >>= 32;
      held -= 32;
    }
  };

  clear();
  if (s == 0) put(LZW_CLEAR, 9);
  int prefix = -1, free_code = LZW_FIRST, width = 9;
  for (int c0 = 0; c0 < pixels; c0 += LZW_CHUNK) {
    const int m = min(LZW_CHUNK, pixels - c0);
    __syncthreads();
    for (int i = lane; i < m; i += 64) pix[i] = src[c0 + i];
    __syncthreads();
    for (int j = 0; j < m; ++j) {                          // every lane walks the same chain: nothing below diverges
      const u32 k = pix[j];
      if (prefix < 0) { prefix = (int)k; continue; }
      const u32 key = ((u32)prefix << 8) | k;
      u32 at = (key * 0x9E3779B1u) >> 19;
      int found = -1;
      for (;;) {
        const u32 e = tab[at];
        if (e == 0) break;
        if ((e >> 12) == key) { found = (int)(e & 4095u); break; }
        at = (at + 1) & (LZW_SLOTS - 1);
      }
      if (found >= 0) { prefix = found; continue; }
      put((u32)prefix, width);
      tab[at] = (key << 12) | (u32)free_code;              // (all lanes store the same word)
      ++free_code;
      if (free_code > (1 << width)) ++width;
      if (free_code == LZW_END) {
        put(LZW_CLEAR, 12);
        clear();
        free_code = LZW_FIRST;
        width = 9;
      }
      prefix = (int)k;
    }
  }
  put((u32)prefix, width);
  ++free_code;                                             // the entry the decoder makes of this code
  if (free_code > (1 << width)) ++width;
  put(s + 1 == strips ? LZW_EOI : LZW_CLEAR, width);
  if (lane == 0) {
    if (held > 0) dst[word] = (u32)acc;
    bits_out[bid] = total;
  }
}

// offs[f][k] = bits before strip k; data_bytes[f]; the 08 in front, the terminator behind, out_len
__global__ __launch_bounds__(256) void gif_scan_kernel(const int *__restrict__ bits, int strips, int *__restrict__ offs,
                                                       int *__restrict__ data_bytes, u8 *__restrict__ out, int64_t cap,
                                                       int *__restrict__ out_len) {
  __shared__ int wave_tot[4];
  const int64_t f = blockIdx.x;
  const int running = carried_exclusive_sum(
      wave_tot, strips, 0, [&](int k) { return bits[f * strips + k]; }, [&](int k, int before) { offs[f * strips + k] = before; });
  if (threadIdx.x == 0) {
    const int nbytes = (running + 7) >> 3, blocks = (nbytes + 254) / 255;
    data_bytes[f] = nbytes;
    out[f * cap] = 8;
    out[f * cap + 1 + nbytes + blocks] = 0;
    out_len[f] = 2 + nbytes + blocks;
  }
}

// grid: one workgroup of 256 per (frame, strip)
__global__ __launch_bounds__(256) void gif_place_kernel(const u8 *__restrict__ stage, int64_t slot_bytes, const int *__restrict__ bits,
                                                        const int *__restrict__ offs, const int *__restrict__ data_bytes, int strips,
                                                        u8 *__restrict__ out, int64_t cap) {
  const int64_t bid = blockIdx.x;
  const int s = (int)(bid % strips);
  const int64_t f = bid / strips;
  const int start = offs[bid], len = bits[bid], nbytes = data_bytes[f];
  const u32 *own = (const u32 *)(stage + bid * slot_bytes);
  const u32 *next = (const u32 *)(stage + (bid + 1) * slot_bytes);
  u8 *dst = out + f * cap;
  const int j1 = (start + len - 1) >> 3;
  for (int j = ((start + 7) >> 3) + threadIdx.x; j <= j1; j += 256) {
    const int p = 8 * j - start, avail = len - p;
    u32 v = bits8(own, p);
    if (avail < 8) {
      v &= (1u << avail) - 1;
      if (s + 1 < strips) v |= (next[0] << avail) & 255u;   // (a strip holds at least two codes: 18 bits)
    }
    const int blk = j / 255;
    dst[2 + j + blk] = (u8)v;
    if (j - blk * 255 == 0) dst[1 + 256 * blk] = (u8)min(255, nbytes - 255 * blk);
  }
}

struct GifLayout {
  int strips, strip_pixels;
  size_t hist, svt, table, nbox, ints, stage, total;
  int64_t slot;
};

// ws: histograms | summed-volume tables | bin tables | boxes in use | bits, offsets, byte counts | staging slots
bool gif_layout(int n, int h, int w, int strip_rows, GifLayout &L) {
  if (n <= 0 || !gif_dims_ok(h, w) || strip_rows < 1) return false;
  const int rows = strip_rows < h ? strip_rows : h;
  L.strips = (h + rows - 1) / rows;
  L.strip_pixels = rows * w;
  L.slot = slot_bytes_of(L.strip_pixels);
  L.hist = 0;
  L.svt = L.hist + (size_t)n * HIST_BYTES;
  L.table = L.svt + (size_t)n * SVT_BYTES;
  L.nbox = L.table + (size_t)n * TABLE_BYTES;
  L.ints = L.nbox + align256(sizeof(int) * (size_t)n);
  L.stage = L.ints + align256(sizeof(int) * ((size_t)2 * n * L.strips + n));
  L.total = L.stage + (size_t)n * L.strips * (size_t)L.slot;
  return true;
}

}  // namespace

extern "C" size_t sp_gif_ws_bytes(int n, int h, int w, int strip_rows) {
  GifLayout L;
  return gif_layout(n, h, w, strip_rows, L) ? L.total : 0;
}

// Bits of one frame: the opening CLEAR, 9; a code per pixel at most, 12 bits at most; a CLEAR, 12 bits, when 3838 codes have
// filled a dictionary (a strip of P pixels sees at most floor(P / 3838) of them, all strips together floor(h*w / 3838)); one
// CLEAR or EOI of at most 12 bits at the end of every strip.  Rounded up to bytes; then one length byte per 255 of them, the
// 08 in front and the terminator.
extern "C" size_t sp_gif_stream_bytes(int h, int w, int strip_rows) {
  if (!gif_dims_ok(h, w) || strip_rows < 1) return 0;
  const int64_t pixels = (int64_t)h * w, rows = strip_rows < h ? strip_rows : h, strips = (h + rows - 1) / rows;
  const int64_t bits = 9 + 12 * pixels + 12 * (pixels / LZW_ENTRIES) + 12 * strips;
  const int64_t bytes = (bits + 7) / 8;
  return (size_t)(1 + bytes + (bytes + 254) / 255 + 1);
}

extern "C" int sp_gif_quantise_u8(const void *frames, int n, int h, int w, void *palette, void *indices, void *ws, size_t ws_bytes,
                                  void *stream) {
  SP_REQUIRE(frames && palette && indices && ws, "sp_gif_quantise_u8: null pointer");
  SP_REQUIRE(n > 0 && gif_dims_ok(h, w), "sp_gif_quantise_u8: n must be positive, h and w in 1..65535 and h*w <= 2^24 (n=%d, %dx%d)",
             n, h, w);
  GifLayout L;
  gif_layout(n, h, w, h, L);
  SP_REQUIRE(ws_bytes >= L.ints, "sp_gif_quantise_u8: ws holds %zu bytes, the quantiser needs %zu (sp_gif_ws_bytes)", ws_bytes, L.ints);
  SP_REQUIRE((uintptr_t)ws % 8 == 0, "sp_gif_quantise_u8: ws must be 8-byte aligned");
  const int64_t total = (int64_t)n * h * w, blocks = (total + 1023) / 1024;
  SP_REQUIRE(blocks <= 0x7fffffff && (int64_t)n * 128 <= 0x7fffffff, "sp_gif_quantise_u8: too many pixels (%lld)", (long long)total);
  hipStream_t s = (hipStream_t)stream;
  u8 *base = (u8 *)ws;
  u64 *hist = (u64 *)(base + L.hist);
  u32 *svt = (u32 *)(base + L.svt);
  u8 *table = base + L.table;
  int *nbox = (int *)(base + L.nbox);
  SP_CLEAR_STALE_ERROR();
  if (hipMemsetAsync(hist, 0, (size_t)n * HIST_BYTES, s) != hipSuccess) {
    sp_set_error("sp_gif_quantise_u8: clearing the histograms failed");
    return SP_ELAUNCH;
  }
  const int hw = h * w;
  hipLaunchKernelGGL(gif_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const u8 *)frames, total, hw,
                     (int)((uintptr_t)frames % 4 == 0), hist);
  hipLaunchKernelGGL(gif_svt_kernel, dim3((unsigned)n * 4), dim3(1024), 0, s, (const u64 *)hist, svt, (int64_t)(SVT_BYTES / sizeof(u32)));
  hipLaunchKernelGGL(gif_split_kernel, dim3((unsigned)n), dim3(256), 0, s, (const u32 *)svt, (int64_t)(SVT_BYTES / sizeof(u32)),
                     (u8 *)palette, nbox);
  hipLaunchKernelGGL(gif_table_kernel, dim3((unsigned)n * 128), dim3(256), 0, s, (const u64 *)hist, (const u8 *)palette,
                     (const int *)nbox, table);
  hipLaunchKernelGGL(gif_map_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const u8 *)frames, total, hw,
                     (int)((uintptr_t)frames % 4 == 0), (int)((uintptr_t)indices % 4 == 0), (const u8 *)table, (u8 *)indices);
  SP_CHECK_LAUNCH("sp_gif_quantise_u8");
  return SP_OK;
}

extern "C" int sp_gif_lzw(const void *indices, int n, int h, int w, int strip_rows, void *out, size_t cap, void *out_len, void *ws,
                          size_t ws_bytes, void *stream) {
  SP_REQUIRE(indices && out && out_len && ws, "sp_gif_lzw: null pointer");
  SP_REQUIRE(n > 0 && gif_dims_ok(h, w), "sp_gif_lzw: n must be positive, h and w in 1..65535 and h*w <= 2^24 (n=%d, %dx%d)", n, h, w);
  SP_REQUIRE(strip_rows >= 1, "sp_gif_lzw: strip_rows %d is not positive", strip_rows);
  GifLayout L;
  gif_layout(n, h, w, strip_rows, L);
  const size_t need = sp_gif_stream_bytes(h, w, strip_rows);
  SP_REQUIRE(cap >= need, "sp_gif_lzw: cap is %zu bytes per frame, a frame can need %zu (sp_gif_stream_bytes)", cap, need);
  SP_REQUIRE(ws_bytes >= L.total, "sp_gif_lzw: ws holds %zu bytes, needs %zu (sp_gif_ws_bytes)", ws_bytes, L.total);
  SP_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)out_len % 4 == 0, "sp_gif_lzw: ws must be 8-byte and out_len 4-byte aligned");
  const int64_t grid = (int64_t)n * L.strips;
  SP_REQUIRE(grid <= 0x7fffffff, "sp_gif_lzw: too many strips (%lld)", (long long)grid);
  hipStream_t s = (hipStream_t)stream;
  u8 *base = (u8 *)ws;
  int *bits = (int *)(base + L.ints), *offs = bits + grid, *data_bytes = offs + grid;
  u8 *stage = base + L.stage;
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(gif_lzw_kernel, dim3((unsigned)grid), dim3(64), 0, s, (const u8 *)indices, h, w, strip_rows < h ? strip_rows : h,
                     L.strips, stage, L.slot, bits);
  hipLaunchKernelGGL(gif_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, (const int *)bits, L.strips, offs, data_bytes, (u8 *)out,
                     (int64_t)cap, (int *)out_len);
  hipLaunchKernelGGL(gif_place_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const u8 *)stage, L.slot, (const int *)bits,
                     (const int *)offs, (const int *)data_bytes, L.strips, (u8 *)out, (int64_t)cap);
  SP_CHECK_LAUNCH("sp_gif_lzw");
  return SP_OK;
}
