// Frame-rate doubling of 8-bit frames (include/svdpipe.h: sp_interp_*): luma planes, the bilateral block motion search, the
// 3x3 vector median, and the overlapped compensation.  Integer arithmetic throughout; tests/interp_model.py is the statement.
//
// The search is the work: per 8x8 block (2R+1)^2 candidates of 256 byte differences.  A workgroup owns one block of one
// pair.  Luma planes are stored replicate-padded by P = R + 4 (the model's clamp acts on the displaced coordinate, so a
// read of the padded plane IS the clamped read), which puts the (16 + 2R)^2 region that all candidates of block (by, bx)
// read at padded (8 by, 8 bx): dword-aligned, staged once per frame of the pair into LDS.  One candidate per lane: a row of
// the 16x16 window is 16 bytes at byte offset R -+ vx, fetched as five aligned dwords and put together with v_alignbyte_b32,
// then four v_sad_u8 per row.  Lanes of a wave hold consecutive vx (and at most three vy), so a wave's reads of one row
// touch a few neighbouring dwords of at most three LDS rows: broadcasts, no conflicts to speak of.
#include "common.h"

namespace {

constexpr int kMaxRange = 24;
constexpr int kMaxDim = 16384;          // h, w
constexpr int kMaxFrames = 32768;       // n (pairs are a grid's z)
constexpr int kSearchThreads = 256;

struct Geometry {
  int pad, ph, pw;                      // border, padded plane rows and pitch (a multiple of 4)
  int64_t plane;                        // bytes per plane
  int bh, bw;
  size_t luma_bytes, raw_bytes;         // the two parts of the workspace
};

__host__ bool geometry(int n, int h, int w, int range, Geometry &g) {
  if (n < 2 || n > kMaxFrames || h < 16 || w < 16 || h > kMaxDim || w > kMaxDim || h % 8 || w % 8 || range < 1 ||
      range > kMaxRange)
    return false;
  g.pad = range + 4;
  g.ph = h + 2 * g.pad;
  g.pw = (w + 2 * g.pad + 3) & ~3;
  g.plane = (int64_t)g.ph * g.pw;
  g.bh = h / 8;
  g.bw = w / 8;
  g.luma_bytes = ((size_t)n * (size_t)g.plane + 15) & ~(size_t)15;
  g.raw_bytes = (size_t)(n - 1) * g.bh * g.bw * 4;
  return true;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// frames uint8 [n][h][w][3] -> planes uint8 [n][ph][pw], replicate-padded.  One thread per dword of a plane.
__global__ __launch_bounds__(256) void luma_kernel(const unsigned char *__restrict__ frames, unsigned *__restrict__ planes, int h,
                                                   int w, int pad, int ph, int pw4) {
  const int x4 = blockIdx.x * blockDim.x + threadIdx.x;
  if (x4 >= pw4) return;
  const int py = blockIdx.y, f = blockIdx.z;
  const unsigned char *row = frames + ((int64_t)f * h + clampi(py - pad, 0, h - 1)) * (int64_t)w * 3;
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned char *p = row + clampi(x4 * 4 + k - pad, 0, w - 1) * 3;
    v |= ((77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8) << (8 * k);
  }
  planes[((int64_t)f * ph + py) * pw4 + x4] = v;
}

// 16 bytes from byte offset `off` of an LDS row of dwords: five aligned dwords, shifted together.
__device__ __forceinline__ void row16(const unsigned *row, int off, unsigned (&d)[4]) {
  const unsigned *q = row + (off >> 2);
  const unsigned s = (unsigned)off & 3;
  const unsigned a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4];
  d[0] = __builtin_amdgcn_alignbyte(a1, a0, s);
  d[1] = __builtin_amdgcn_alignbyte(a2, a1, s);
  d[2] = __builtin_amdgcn_alignbyte(a3, a2, s);
  d[3] = __builtin_amdgcn_alignbyte(a4, a3, s);
}

// grid (bw, bh, n - 1).  LDS: two regions of S = 16 + 2R rows, each row lp4 dwords (>= (S + 4) / 4, so that the fifth dword
// of row16 at the largest offset, bytes 2R + 16 .. 2R + 19, is inside the row), then one key per wave.
__global__ __launch_bounds__(kSearchThreads) void search_kernel(const unsigned *__restrict__ planes, short *__restrict__ raw, int range,
                                                                int lam, int64_t plane4, int pw4, int lp4) {
  extern __shared__ unsigned lds[];
  const int S = 16 + 2 * range, side = 2 * range + 1;
  const int bx = blockIdx.x, by = blockIdx.y, pair = blockIdx.z;
  unsigned *ra = lds, *rb = lds + S * lp4;
  unsigned *wave_key = rb + S * lp4;

  // the region's top-left in a padded plane is (8 by, 8 bx); its rows end at most at column w + 2 pad <= pitch
  const int src4 = (S + 3) >> 2;        // dwords of a row that hold region bytes; the rest of the LDS row is zero
  const unsigned *ga = planes + (int64_t)pair * plane4 + (int64_t)(8 * by) * pw4 + 2 * bx;
  const unsigned *gb = ga + plane4;
  for (int i = threadIdx.x; i < S * lp4; i += kSearchThreads) {
    const int r = i / lp4, c = i - r * lp4;
    const bool in = c < src4;
    ra[i] = in ? ga[(int64_t)r * pw4 + c] : 0u;
    rb[i] = in ? gb[(int64_t)r * pw4 + c] : 0u;
  }
  __syncthreads();

  unsigned best = 0xffffffffu;
  for (int idx = threadIdx.x; idx < side * side; idx += kSearchThreads) {
    const int cy = idx / side, cx = idx - cy * side;      // vy + R, vx + R
    const int vy = cy - range, vx = cx - range;
    // window row r, column c: A at region (R - vy + r, R - vx + c), B at (R + vy + r, R + vx + c)
    const unsigned *pa = ra + (2 * range - cy) * lp4;
    const unsigned *pb = rb + cy * lp4;
    const int oa = 2 * range - cx, ob = cx;
    unsigned sad = 0;
#pragma unroll 4
    for (int r = 0; r < 16; ++r) {
      unsigned a[4], b[4];
      row16(pa + r * lp4, oa, a);
      row16(pb + r * lp4, ob, b);
#pragma unroll
      for (int k = 0; k < 4; ++k) sad = __builtin_amdgcn_sad_u8(a[k], b[k], sad);
    }
    const unsigned cost = sad + (unsigned)(lam * (abs(vy) + abs(vx)));      // < 2^17
    best = min(best, (cost << 12) | (unsigned)idx);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 64));
  if ((threadIdx.x & 63) == 0) wave_key[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned k = wave_key[0];
#pragma unroll
    for (int i = 1; i < kSearchThreads / 64; ++i) k = min(k, wave_key[i]);
    const int idx = (int)(k & 4095u);
    short *dst = raw + (((int64_t)pair * gridDim.y + by) * gridDim.x + bx) * 2;
    dst[0] = (short)(idx / side - range);
    dst[1] = (short)(idx % side - range);
  }
}

// 5th smallest of nine: a partial selection sort (the five least, in order)
__device__ __forceinline__ int median9(int (&v)[9]) {
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = i + 1; j < 9; ++j) {
      const int lo = min(v[i], v[j]), hi = max(v[i], v[j]);
      v[i] = lo;
      v[j] = hi;
    }
  return v[4];
}

// raw -> vectors, both int16 [pairs][bh][bw][2]; one thread per block
__global__ __launch_bounds__(256) void median_kernel(const short *__restrict__ raw, short *__restrict__ vectors, int bh, int bw,
                                                     int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int bx = (int)(i % bw), by = (int)(i / bw % bh);
  const short *grid = raw + (i / ((int64_t)bh * bw)) * (int64_t)bh * bw * 2;
  int vy[9], vx[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const short *p = grid + ((int64_t)clampi(by + k / 3 - 1, 0, bh - 1) * bw + clampi(bx + k % 3 - 1, 0, bw - 1)) * 2;
    vy[k] = p[0];
    vx[k] = p[1];
  }
  vectors[i * 2] = (short)median9(vy);
  vectors[i * 2 + 1] = (short)median9(vx);
}

// out [2n - 1][h][w][3]: even frames are copies, odd frames the overlapped blend of their neighbours.  One thread per pixel.
__global__ __launch_bounds__(256) void compensate_kernel(const unsigned char *__restrict__ frames, const short *__restrict__ vectors,
                                                         unsigned char *__restrict__ out, int h, int w) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= w) return;
  const int y = blockIdx.y, fo = blockIdx.z;
  const int64_t frame = (int64_t)h * w * 3;
  unsigned char *dst = out + fo * frame + ((int64_t)y * w + x) * 3;
  const unsigned char *a = frames + (fo >> 1) * frame;
  if (!(fo & 1)) {
    const unsigned char *src = a + ((int64_t)y * w + x) * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    return;
  }
  const unsigned char *b = a + frame;
  const int bh = h >> 3, bw = w >> 3;
  const short *grid = vectors + (int64_t)(fo >> 1) * bh * bw * 2;
  const int ty = y + 4, tx = x + 4;
  const int by0 = (ty >> 3) - 1, bx0 = (tx >> 3) - 1;
  const int wy1 = 2 * (ty & 7) + 1, wx1 = 2 * (tx & 7) + 1;
  int acc[3] = {256, 256, 256};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int dy = k >> 1, dx = k & 1;
    const short *v = grid + ((int64_t)clampi(by0 + dy, 0, bh - 1) * bw + clampi(bx0 + dx, 0, bw - 1)) * 2;
    const int vy = v[0], vx = v[1];
    const int wgt = (dy ? wy1 : 16 - wy1) * (dx ? wx1 : 16 - wx1);
    const unsigned char *pa = a + ((int64_t)clampi(y - vy, 0, h - 1) * w + clampi(x - vx, 0, w - 1)) * 3;
    const unsigned char *pb = b + ((int64_t)clampi(y + vy, 0, h - 1) * w + clampi(x + vx, 0, w - 1)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += wgt * ((int)pa[c] + (int)pb[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c] = (unsigned char)(acc[c] >> 9);
}

}  // namespace

extern "C" size_t sp_interp_ws_bytes(int n, int h, int w, int range) {
  Geometry g;
  return geometry(n, h, w, range, g) ? g.luma_bytes + g.raw_bytes : 0;
}

#define SP_INTERP_DIMS(name, n, h, w)                                                                                    \
  SP_REQUIRE(n >= 2 && n <= kMaxFrames, "%s: n = %d must be 2..%d frames", name, n, kMaxFrames);                           \
  SP_REQUIRE(h >= 16 && w >= 16 && h <= kMaxDim && w <= kMaxDim && h % 8 == 0 && w % 8 == 0,                              \
             "%s: h = %d and w = %d must be multiples of 8 from 16 to %d", name, h, w, kMaxDim)

extern "C" int sp_interp_motion_u8(const void *frames, int n, int h, int w, int range, int lam, void *vectors, void *raw_vectors,
                                   void *ws, size_t ws_bytes, void *stream) {
  const char *name = "sp_interp_motion_u8";
  SP_REQUIRE(frames && vectors && ws, "%s: null pointer", name);
  SP_INTERP_DIMS(name, n, h, w);
  SP_REQUIRE(range >= 1 && range <= kMaxRange, "%s: range = %d must be 1..%d", name, range, kMaxRange);
  SP_REQUIRE(lam >= 0 && lam <= 255, "%s: lam = %d must be 0..255", name, lam);
  SP_REQUIRE((uintptr_t)vectors % 2 == 0 && (uintptr_t)raw_vectors % 2 == 0, "%s: vectors must be 2-byte aligned", name);
  SP_REQUIRE((uintptr_t)ws % 4 == 0, "%s: ws must be 4-byte aligned", name);
  Geometry g;
  geometry(n, h, w, range, g);
  SP_REQUIRE(ws_bytes >= g.luma_bytes + g.raw_bytes, "%s: ws_bytes = %zu is below sp_interp_ws_bytes = %zu", name, ws_bytes,
             g.luma_bytes + g.raw_bytes);
  hipStream_t s = (hipStream_t)stream;
  unsigned *planes = (unsigned *)ws;
  short *raw = raw_vectors ? (short *)raw_vectors : (short *)((char *)ws + g.luma_bytes);
  const int pw4 = g.pw / 4;
  const int S = 16 + 2 * range, lp4 = (S + 4 + 3) / 4;
  const size_t lds = ((size_t)2 * S * lp4 + kSearchThreads / 64) * 4;       // 8.7 KB at R = 24
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(luma_kernel, dim3((pw4 + 255) / 256, g.ph, n), dim3(256), 0, s, (const unsigned char *)frames, planes, h, w,
                     g.pad, g.ph, pw4);
  SP_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(search_kernel, dim3(g.bw, g.bh, n - 1), dim3(kSearchThreads), lds, s, (const unsigned *)planes, raw, range,
                     lam, g.plane / 4, pw4, lp4);
  SP_CHECK_LAUNCH(name);
  const int64_t total = (int64_t)(n - 1) * g.bh * g.bw;
  hipLaunchKernelGGL(median_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const short *)raw, (short *)vectors,
                     g.bh, g.bw, total);
  SP_CHECK_LAUNCH(name);
  return SP_OK;
}

extern "C" int sp_interp_compensate_u8(const void *frames, int n, int h, int w, const void *vectors, void *out, void *stream) {
  const char *name = "sp_interp_compensate_u8";
  SP_REQUIRE(frames && vectors && out, "%s: null pointer", name);
  SP_INTERP_DIMS(name, n, h, w);
  SP_REQUIRE((uintptr_t)vectors % 2 == 0, "%s: vectors must be 2-byte aligned", name);
  const size_t in_bytes = (size_t)n * h * w * 3, out_bytes = (size_t)(2 * n - 1) * h * w * 3;
  SP_REQUIRE((uintptr_t)out + out_bytes <= (uintptr_t)frames || (uintptr_t)frames + in_bytes <= (uintptr_t)out,
             "%s: out must not overlap frames", name);
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(compensate_kernel, dim3((w + 255) / 256, h, 2 * n - 1), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char *)frames, (const short *)vectors, (unsigned char *)out, h, w);
  SP_CHECK_LAUNCH(name);
  return SP_OK;
}
