// FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net") on an up resnet's concatenation buffer, IN PLACE, for gfx950
// (DESIGN.md section 27).  cat: fp16 rows [n_img*h*w][c_left + c_right], the running tensor h in columns [0, c_left), the
// skip in [c_left, c_left + c_right); image i owns rows i*h*w .. (i+1)*h*w - 1.
//
//  * Backbone scale, columns [0, c_left/2): version 1 multiplies by b; version 2 by (b - 1)*mhat[p] + 1 with m[p] the mean
//    of pixel p over all c_left channels (before any scaling) and mhat = (m - lo)/(hi - lo) over the image's pixels;
//    hi == lo gives mhat = 0 (factor 1), where the widespread implementation divides 0 by 0.
//  * Skip filter, columns [c_left, c_left + c_right): ifftn(ifftshift(fftshift(fftn(x)) * mask)).real with mask = s on the
//    2 x 2 block of frequencies {-1, 0} x {-1, 0} and 1 elsewhere.  For a real image that is the input plus a rank-7
//    projection, per image and channel (ay = 2 pi y / H, ax = 2 pi x / W):
//        out[n] = x[n] + (s - 1)/(H W) * sum_j phi_j(n) coef_j,      coef_j = sum_m phi_j(m) x[m]
//        phi = { 1, cos ay, sin ay, cos ax, sin ax, cos(ay + ax), sin(ay + ax) }
//    so no FFT and no complex arithmetic: seven fp32 sums per (image, channel) and one fused update.
//
// Three launches, no atomics, every sum folded in a fixed order (the same bytes on every run and under graph replay):
//  1. freeu_mean_kernel (version 2, b != 1): workgroup = 32 consecutive rows of one image; a row is summed by lpr = 8 .. 64
//     lanes (16-byte loads, eight sequential fp32 adds per piece, then an xor tree over the lpr lanes); m[row] and the
//     workgroup's (min, max) go to the workspace.
//  2. freeu_coef_kernel (s != 1): grid = (image, 64-channel slab, token chunk), workgroup = 32 row lanes x 8 channel lanes:
//     the 8 channel lanes of a row lane read one whole 128-byte line.  cos / sin of ay and of ax come from LDS tables built
//     once per workgroup (sincospif of an argument in [-1, 1]); cos(ay + ax), sin(ay + ax) by the addition formulas; (y, x)
//     advance without a division.  7 x 8 fp32 accumulators per thread; reduced over the 8 row lanes of a wave by xor 8, 16,
//     32, over the 4 waves through LDS in wave order; one [7][64] partial per workgroup goes to the workspace.
//  3. freeu_apply_kernel: the same (image, slab, chunk) grid over the right half plus the slabs of the left half's first
//     c_left/2 channels.  A right-half workgroup adds its (image, slab)'s partials in chunk order, times (s - 1)/(H W), keeps
//     its thread's 7 x 8 coefficients in registers and streams its chunk: x + sum_j phi_j coef_j in fp32, one rounding.  A
//     left-half workgroup folds the image's (min, max) partials (exact: no rounding in min / max) and multiplies.
// s == 1 launches no coefficient pass and no right-half workgroup, b == 1 no mean pass and no left-half workgroup: those
// columns keep their bytes (x + 0 would turn -0 into +0).  Nothing outside columns [0, c_left/2) and [c_left, c_left +
// c_right) of rows [0, n_img*h*w) is written; nothing outside the buffer's c_left + c_right columns of those rows is read.
#include <float.h>
#include "common.h"

namespace {

constexpr int FU_SLAB = 64;          // channels per slab: 8 channel lanes x 16 bytes = one 128-byte line per row
constexpr int FU_ROWS = 32;          // row lanes per workgroup (coefficient and apply passes); rows per mean workgroup
constexpr int FU_NPHI = 7;
constexpr int FU_PART = FU_NPHI * FU_SLAB;   // floats per coefficient partial
constexpr int FU_MAX_CHUNKS = 64;    // token chunks per image at most (the apply pass adds that many partials per coefficient)
constexpr int FU_CHUNK_MIN = 256;    // ... of at least this many rows
constexpr int FU_TARGET_WGS = 1024;  // workgroups the coefficient pass aims at: four per CU
constexpr int FU_MAX_HW = 4096;      // h + w at most: the cos / sin tables take 8*(h + w) bytes of LDS
constexpr int FU_MAX_C = 1 << 30;    // c_left, c_right at most: a column index rounded up to a slab stays in 32 bits

struct FreeuPlan {
  int hw, rslabs, lslabs, nchunks, chunk_rows, mean_blocks, lpr;
  size_t off_minmax, off_coef, total;
};

// The split of one call and its workspace: [n_img*hw] fp32 means, [n_img][mean_blocks][2] fp32 (min, max),
// [n_img][rslabs][nchunks][7][64] fp32 coefficient partials.  false: a shape the call refuses.
bool freeu_plan(int n_img, int h, int w, int c_left, int c_right, FreeuPlan &p) {
  if (n_img <= 0 || h < 2 || w < 2 || c_left <= 0 || c_right <= 0 || c_left % 16 || c_right % 8) return false;
  if ((int64_t)h + w > FU_MAX_HW || c_left > FU_MAX_C || c_right > FU_MAX_C) return false;
  const int64_t hw = (int64_t)h * w, rows = hw * n_img;
  if (rows > 0x7fffffff - 2 * FU_ROWS) return false;                    // (row indices rounded up to a block stay in 32 bits)
  p.hw = (int)hw;
  p.rslabs = (c_right + FU_SLAB - 1) / FU_SLAB;
  p.lslabs = (c_left / 2 + FU_SLAB - 1) / FU_SLAB;
  const int64_t per_chunk = (int64_t)n_img * p.rslabs;
  int64_t want = (FU_TARGET_WGS + per_chunk - 1) / per_chunk;
  const int64_t cap = (hw + FU_CHUNK_MIN - 1) / FU_CHUNK_MIN;
  if (want > cap) want = cap;
  if (want > FU_MAX_CHUNKS) want = FU_MAX_CHUNKS;
  if (want < 1) want = 1;
  const int64_t chunk_rows = ((hw + want - 1) / want + FU_ROWS - 1) / FU_ROWS * FU_ROWS;
  p.chunk_rows = (int)chunk_rows;
  p.nchunks = (int)((hw + chunk_rows - 1) / chunk_rows);
  p.mean_blocks = (int)((hw + FU_ROWS - 1) / FU_ROWS);
  const int pieces = c_left / 8;
  p.lpr = pieces > 32 ? 64 : pieces > 16 ? 32 : pieces > 8 ? 16 : 8;
  if ((int64_t)n_img * (p.rslabs + p.lslabs) * p.nchunks > 0x7fffffff || (int64_t)n_img * p.mean_blocks > 0x7fffffff) return false;
  p.off_minmax = (size_t)rows * 4;
  p.off_coef = p.off_minmax + (size_t)n_img * p.mean_blocks * 8;
  p.total = p.off_coef + (size_t)n_img * p.rslabs * p.nchunks * FU_PART * 4;
  return true;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// cos and sin of 2 pi i / n for i = 0 .. n - 1; the argument of sincospif is (2i - 2n)/n or 2i/n, whichever lies in [-1, 1]
__device__ __forceinline__ void freeu_table(float *c, float *s, int n, int tid) {
  for (int i = tid; i < n; i += 256) {
    const int k = 2 * i > n ? 2 * i - 2 * n : 2 * i;
    sincospif((float)k / (float)n, &s[i], &c[i]);
  }
}

// ------------------------------------------------------------------------------------------------
// grid.x = image major, block of 32 rows minor
__global__ __launch_bounds__(256) void freeu_mean_kernel(const f16 *__restrict__ cat, int64_t ld, int hw, int c_left, int lpr,
                                                         int mean_blocks, float *__restrict__ mean, float *__restrict__ minmax) {
  __shared__ float red[8];
  const int tid = threadIdx.x;
  const int img = blockIdx.x / mean_blocks, blk = blockIdx.x - img * mean_blocks;
  const int sub = tid & (lpr - 1), rg = tid / lpr, per_pass = 256 / lpr, pieces = c_left / 8;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int r = rg; r < FU_ROWS; r += per_pass) {
    const int row = blk * FU_ROWS + r;
    float sum = 0.f;
    if (row < hw) {
      const f16 *p = cat + ((int64_t)img * hw + row) * ld;
      for (int piece = sub; piece < pieces; piece += lpr) {
        const f16x8 v = *(const f16x8 *)(p + piece * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += (float)v[e];
      }
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);     // (lpr divides 64: a row's lanes share a wave)
    if (row < hw) {
      const float m = sum / (float)c_left;
      if (sub == 0) mean[(int64_t)img * hw + row] = m;
      lo = fminf(lo, m);
      hi = fmaxf(hi, m);
    }
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((tid & 63) == 0) { red[tid >> 6] = lo; red[4 + (tid >> 6)] = hi; }
  __syncthreads();
  if (tid == 0) {
    float *mm = minmax + ((int64_t)img * mean_blocks + blk) * 2;
    mm[0] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    mm[1] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  }
}

// ------------------------------------------------------------------------------------------------
// grid.x = ((image, slab), chunk); dynamic LDS: cos ay [h], sin ay [h], cos ax [w], sin ax [w]
__global__ __launch_bounds__(256) void freeu_coef_kernel(const f16 *__restrict__ cat, int64_t ld, int h, int w, int c_left,
                                                         int c_right, int rslabs, int nchunks, int chunk_rows,
                                                         float *__restrict__ part) {
  extern __shared__ float tab[];
  __shared__ float red[4 * FU_PART];
  float *cyt = tab, *syt = tab + h, *cxt = tab + 2 * h, *sxt = tab + 2 * h + w;
  const int tid = threadIdx.x, chl = tid & 7, rl = tid >> 3;
  const int chunk = blockIdx.x % nchunks, is = blockIdx.x / nchunks;
  const int img = is / rslabs, slab = is - img * rslabs;
  const int hw = h * w;
  freeu_table(cyt, syt, h, tid);
  freeu_table(cxt, sxt, w, tid);
  __syncthreads();

  float acc[FU_NPHI][8];
#pragma unroll
  for (int j = 0; j < FU_NPHI; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;

  const int col = slab * FU_SLAB + chl * 8;
  const int r1 = min((chunk + 1) * chunk_rows, hw);
  int row = chunk * chunk_rows + rl;
  if (col < c_right) {                               // (a ragged last slab: the lanes behind c_right add zeros)
    const int dy = FU_ROWS / w, dx = FU_ROWS - dy * w;
    int y = row / w, x = row - y * w;
    const f16 *p = cat + ((int64_t)img * hw + row) * ld + c_left + col;
    const int64_t pstep = (int64_t)FU_ROWS * ld;
    for (; row < r1; row += FU_ROWS, p += pstep) {
      const f16x8 v = *(const f16x8 *)p;
      const float cy = cyt[y], sy = syt[y], cx = cxt[x], sx = sxt[x];
      const float c2 = cy * cx - sy * sx, s2 = sy * cx + cy * sx;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = (float)v[e];
        acc[0][e] += f;
        acc[1][e] = fmaf(cy, f, acc[1][e]);
        acc[2][e] = fmaf(sy, f, acc[2][e]);
        acc[3][e] = fmaf(cx, f, acc[3][e]);
        acc[4][e] = fmaf(sx, f, acc[4][e]);
        acc[5][e] = fmaf(c2, f, acc[5][e]);
        acc[6][e] = fmaf(s2, f, acc[6][e]);
      }
      y += dy;
      x += dx;
      if (x >= w) { x -= w; ++y; }
    }
  }
  // the 8 row lanes of a wave (lane = 8*(rl & 7) + chl), then the 4 waves in wave order
#pragma unroll
  for (int j = 0; j < FU_NPHI; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = acc[j][e];
      v += __shfl_xor(v, 8, 64);
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      acc[j][e] = v;
    }
  if ((tid & 63) < 8) {
    float *dst = red + (tid >> 6) * FU_PART + chl * 8;
#pragma unroll
    for (int j = 0; j < FU_NPHI; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[j * FU_SLAB + e] = acc[j][e];
  }
  __syncthreads();
  float *dst = part + ((int64_t)is * nchunks + chunk) * FU_PART;
  for (int i = tid; i < FU_PART; i += 256)
    dst[i] = ((red[i] + red[FU_PART + i]) + red[2 * FU_PART + i]) + red[3 * FU_PART + i];
}

// ------------------------------------------------------------------------------------------------
// grid.x = ((image, slab), chunk) with slabs 0 .. rs - 1 of the right half (rs = rslabs, or 0 when s == 1) and then ls slabs
// of the left half's first c_left/2 channels (ls = lslabs, or 0 when b == 1).  g = (s - 1)/(h w).
__global__ __launch_bounds__(256) void freeu_apply_kernel(f16 *__restrict__ cat, int64_t ld, int h, int w, int c_left, int c_right,
                                                          int rs, int ls, int rslabs, int nchunks, int chunk_rows,
                                                          const float *__restrict__ part, const float *__restrict__ mean,
                                                          const float *__restrict__ minmax, int mean_blocks, float b, float g,
                                                          int version) {
  extern __shared__ float tab[];
  __shared__ float coef[FU_PART];
  __shared__ float red[8];
  const int tid = threadIdx.x, chl = tid & 7, rl = tid >> 3;
  const int chunk = blockIdx.x % nchunks, is = blockIdx.x / nchunks;
  const int img = is / (rs + ls), slab = is - img * (rs + ls);
  const int hw = h * w;
  const int r1 = min((chunk + 1) * chunk_rows, hw);
  int row = chunk * chunk_rows + rl;
  const int64_t pstep = (int64_t)FU_ROWS * ld;

  if (slab < rs) {                                   // ---- skip filter
    float *cyt = tab, *syt = tab + h, *cxt = tab + 2 * h, *sxt = tab + 2 * h + w;
    freeu_table(cyt, syt, h, tid);
    freeu_table(cxt, sxt, w, tid);
    const float *src = part + ((int64_t)img * rslabs + slab) * nchunks * FU_PART;
    for (int i = tid; i < FU_PART; i += 256) {
      float sum = src[i];
      for (int c = 1; c < nchunks; ++c) sum += src[(int64_t)c * FU_PART + i];
      coef[i] = g * sum;
    }
    __syncthreads();
    const int col = slab * FU_SLAB + chl * 8;
    if (col >= c_right) return;                      // (no barrier below)
    float ck[FU_NPHI][8];
#pragma unroll
    for (int j = 0; j < FU_NPHI; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) ck[j][e] = coef[j * FU_SLAB + chl * 8 + e];
    const int dy = FU_ROWS / w, dx = FU_ROWS - dy * w;
    int y = row / w, x = row - y * w;
    f16 *p = cat + ((int64_t)img * hw + row) * ld + c_left + col;
    for (; row < r1; row += FU_ROWS, p += pstep) {
      const f16x8 v = *(const f16x8 *)p;
      const float cy = cyt[y], sy = syt[y], cx = cxt[x], sx = sxt[x];
      const float c2 = cy * cx - sy * sx, s2 = sy * cx + cy * sx;
      f16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = ck[0][e];
        t = fmaf(cy, ck[1][e], t);
        t = fmaf(sy, ck[2][e], t);
        t = fmaf(cx, ck[3][e], t);
        t = fmaf(sx, ck[4][e], t);
        t = fmaf(c2, ck[5][e], t);
        t = fmaf(s2, ck[6][e], t);
        o[e] = (f16)((float)v[e] + t);               // (one rounding, to nearest even)
      }
      *(f16x8 *)p = o;
      y += dy;
      x += dx;
      if (x >= w) { x -= w; ++y; }
    }
    return;
  }

  // ---- backbone scale
  float lo = 0.f, inv_ok = 0.f, span = 1.f;
  if (version == 2) {
    float l = __builtin_inff(), u = -__builtin_inff();
    const float *mm = minmax + (int64_t)img * mean_blocks * 2;
    for (int i = tid; i < mean_blocks; i += 256) { l = fminf(l, mm[2 * i]); u = fmaxf(u, mm[2 * i + 1]); }
    l = wave_min(l);
    u = wave_max(u);
    if ((tid & 63) == 0) { red[tid >> 6] = l; red[4 + (tid >> 6)] = u; }
    __syncthreads();
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    const float hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    if (hi > lo) { inv_ok = 1.f; span = hi - lo; }   // hi == lo (or a NaN): mhat = 0, the factor is 1
  }
  const int col = (slab - rs) * FU_SLAB + chl * 8;
  if (col >= c_left / 2) return;
  f16 *p = cat + ((int64_t)img * hw + row) * ld + col;
  const float *mp = mean + (int64_t)img * hw;
  for (; row < r1; row += FU_ROWS, p += pstep) {
    float f = b;
    if (version == 2) {
      const float mhat = inv_ok != 0.f ? (mp[row] - lo) / span : 0.f;
      f = fmaf(b - 1.0f, mhat, 1.0f);
    }
    const f16x8 v = *(const f16x8 *)p;
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)((float)v[e] * f);
    *(f16x8 *)p = o;
  }
}

}  // namespace

extern "C" size_t sp_freeu_ws_bytes(int n_img, int h, int w, int c_left, int c_right) {
  FreeuPlan p;
  return freeu_plan(n_img, h, w, c_left, c_right, p) ? p.total : 0;
}

extern "C" int sp_freeu_f16(void *cat, int64_t ld, int n_img, int h, int w, int c_left, int c_right, float b, float s,
                            int version, void *ws, size_t ws_bytes, void *stream) {
  SP_REQUIRE(cat && ws, "sp_freeu_f16: null pointer");
  SP_REQUIRE(n_img > 0 && h > 0 && w > 0 && c_left > 0 && c_right > 0,
             "sp_freeu_f16: n_img %d, h %d, w %d, c_left %d and c_right %d must be positive", n_img, h, w, c_left, c_right);
  SP_REQUIRE(h >= 2 && w >= 2, "sp_freeu_f16: a %d x %d image has no frequency -1 (h and w must be at least 2)", h, w);
  SP_REQUIRE(c_left % 16 == 0 && c_right % 8 == 0, "sp_freeu_f16: c_left %d must be a multiple of 16 and c_right %d of 8",
             c_left, c_right);
  SP_REQUIRE(ld >= (int64_t)c_left + c_right && ld % 8 == 0,
             "sp_freeu_f16: row pitch %lld must be at least c_left + c_right = %lld and a multiple of 8", (long long)ld,
             (long long)c_left + c_right);
  SP_REQUIRE(((uintptr_t)cat & 15) == 0 && ((uintptr_t)ws & 3) == 0, "sp_freeu_f16: cat must be 16-byte and ws 4-byte aligned");
  SP_REQUIRE(version == 1 || version == 2, "sp_freeu_f16: version %d (1 or 2)", version);
  SP_REQUIRE(b > 0.f && b <= FLT_MAX && s > 0.f && s <= FLT_MAX, "sp_freeu_f16: b and s must be positive and finite");
  FreeuPlan p;
  SP_REQUIRE(freeu_plan(n_img, h, w, c_left, c_right, p), "sp_freeu_f16: n_img*h*w, h + w or the channel counts too large");
  SP_REQUIRE(ws_bytes >= p.total, "sp_freeu_f16: ws_bytes = %zu is below sp_freeu_ws_bytes = %zu", ws_bytes, p.total);

  const int rs = s != 1.0f ? p.rslabs : 0, ls = b != 1.0f ? p.lslabs : 0;
  if (rs + ls == 0) return SP_OK;                    // b = s = 1: the identity
  hipStream_t st = (hipStream_t)stream;
  f16 *x = (f16 *)cat;
  float *mean = (float *)ws, *minmax = (float *)((char *)ws + p.off_minmax), *part = (float *)((char *)ws + p.off_coef);
  const size_t lds = (size_t)2 * (h + w) * sizeof(float);
  SP_CLEAR_STALE_ERROR();
  if (ls && version == 2) {
    hipLaunchKernelGGL(freeu_mean_kernel, dim3((unsigned)(n_img * p.mean_blocks)), dim3(256), 0, st, (const f16 *)x, ld, p.hw,
                       c_left, p.lpr, p.mean_blocks, mean, minmax);
    SP_CHECK_LAUNCH("sp_freeu_f16");
  }
  if (rs) {
    hipLaunchKernelGGL(freeu_coef_kernel, dim3((unsigned)(n_img * p.rslabs * p.nchunks)), dim3(256), lds, st, (const f16 *)x, ld, h,
                       w, c_left, c_right, p.rslabs, p.nchunks, p.chunk_rows, part);
    SP_CHECK_LAUNCH("sp_freeu_f16");
  }
  hipLaunchKernelGGL(freeu_apply_kernel, dim3((unsigned)(n_img * (rs + ls) * p.nchunks)), dim3(256), lds, st, x, ld, h, w, c_left,
                     c_right, rs, ls, p.rslabs, p.nchunks, p.chunk_rows, (const float *)part, (const float *)mean,
                     (const float *)minmax, p.mean_blocks, b, (s - 1.0f) / (float)p.hw, version);
  SP_CHECK_LAUNCH("sp_freeu_f16");
  return SP_OK;
}
