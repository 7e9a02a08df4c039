// The sampler tails behind the UNet's stored eps rows, one kernel: the Euler update of the latent (B,4,F,H,W) or the
// DPM-Solver++(2M) update of the state (B,8,F,H,W: channels 0-3 the sample x, channels 4-7 the previous step's denoised
// estimate, the solver's history riding in the latent itself), each behind one set of eps rows [B][F][H*W][ld_eps] or behind
// overlapping frame windows (temporal co-denoising): a latent of F_total frames cut into n_win windows of `window` frames,
// `stride` apart, the UNet run once per window, the eps rows of all windows in one buffer [n_win][B][window][H*W][ld_eps],
// blended frame by frame with the host's normalised weight table in front of ONE update of the whole latent.  The arithmetic
// is that of sampler_math.h.  See sp_euler_step_rows_f16 ... sp_dpmpp2m_step_windows_f16 in svdpipe.h.  The stochastic
// samplers (sp_euler_ancestral_step_f16, sp_dpmpp2m_sde_step_f16) are the same kernel with NOISE: behind the window loop it
// evaluates the step's normals of its elements from the video's seed (noise.h) and adds n*z inside the update.
// Large frames (sp_euler_step_tiles_f16, sp_dpmpp2m_step_tiles_f16) are the same kernel with PLAN = TILES: the frame windows
// times overlapping spatial tiles of tile_h x tile_w cells, the eps rows of all patches in one buffer
// [n_patch][B][window][tile_h*tile_w][ld_eps], patch (kf, ky, kx) at k = (kf*n_ty + ky)*n_tx + kx, blended per pixel with the
// product of three small tables, (wf[kf][p] * wy[ky][y - ky*sy]) * wx[kx][x - kx*sx].
#include "noise.h"
#include "sampler_math.h"

namespace {

struct WindowPlan {
  int frames, window, stride, n_win, batch;   // frames = F_total
};

// The space half of a tile plan: the latent's row length, the tile, the strides, the tile counts and the two axis tables.
struct TileGeom {
  int w, th, tw, sy, sx, n_ty, n_tx;
  const float *wy, *wx;                       // [n_ty][th], [n_tx][tw]
};

enum { EULER = 0, FIRST_ORDER = 1, SECOND_ORDER = 2 };   // FIRST_ORDER: 2M with c2 == 0, the D_prev planes are never read
enum { ROWS = 0, WINDOWS = 1, TILES = 2 };               // what the eps rows are cut into: nothing, frame windows, windows x tiles

// A thread owns PX adjacent pixels of one (b, f): the planes are read and written PX at a time (8 bytes for PX = 4), the eps
// rows one 8-byte row per pixel and covering window.  Every value a thread reads from `st` is in a register before its first
// store and no other thread touches those elements, so out == st (update in place) is safe; hence no __restrict__ on the two.
// PLAN = ROWS is one window that is the whole latent: no weight table, one eps row per pixel at bf * hw + p, guidance
// indexed by the frame; the loop below is then one pass and e the eps itself.
// PLAN = TILES: the covering tiles are those of the thread's first pixel (y, x).  With PX = 4 the host has seen to w, tw and
// sx being multiples of 4, so the four pixels lie in one row, share their covering tiles and have adjacent eps rows inside a
// tile -- or to there being one tile that is the whole frame, whose eps rows are the frame's pixels in order.
// NOISE: z of element (c, f, p) of video b from (seeds[b], step), f the GLOBAL frame: with PX = 4 the thread's four pixels of a
// channel are the four lanes of one block (hw % 4 == 0), with PX = 1 it evaluates its element's block and takes its lane.
template <int PX, int MODE, int PLAN, bool NOISE>
__global__ __launch_bounds__(256) void sampler_tail_kernel(const f16 *st, const f16 *__restrict__ ec,
                                                           const f16 *__restrict__ eu, int64_t ld_eps,
                                                           const float *__restrict__ gs, int64_t ld_g,
                                                           const float *__restrict__ wn, f16 *out, SamplerCoef k,
                                                           WindowPlan wp, TileGeom tg, int64_t hw, int64_t total,
                                                           const uint64_t *__restrict__ seeds, uint32_t step) {
  typedef f16 vec __attribute__((ext_vector_type(PX)));
  constexpr bool WINDOWS = PLAN != ROWS;
  constexpr int CH = MODE == EULER ? 4 : 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one group of PX pixels of a (b, f)
  if (idx >= total) return;
  const int frames = wp.frames;
  const int64_t groups = hw / PX;
  const int64_t p = (idx % groups) * PX;
  const int64_t bf = idx / groups;
  const int f = (int)(bf % frames);
  const int64_t b = bf / frames;
  const int64_t plane0 = (b * CH * frames + f) * hw + p;                 // channel c: + c * frames * hw
  const int64_t cs = (int64_t)frames * hw;

  float x[4][PX], dp[4][PX], e[4][PX];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if constexpr (PX == 1) {
      x[c][0] = (float)st[plane0 + c * cs];
      dp[c][0] = MODE == SECOND_ORDER ? (float)st[plane0 + (4 + c) * cs] : 0.f;
    } else {
      const vec xv = *(const vec *)(st + plane0 + c * cs);
      vec dv = {};
      if (MODE == SECOND_ORDER) dv = *(const vec *)(st + plane0 + (4 + c) * cs);
#pragma unroll
      for (int j = 0; j < PX; ++j) { x[c][j] = (float)xv[j]; dp[c][j] = (float)dv[j]; }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) e[c][j] = 0.f;
  }
  // the windows that cover global frame f, in ascending order: k*stride <= f <= k*stride + window - 1
  int k_lo = 0, k_hi = 0;
  if constexpr (WINDOWS) {
    k_lo = f < wp.window ? 0 : (f - wp.window) / wp.stride + 1;
    k_hi = min(f / wp.stride, wp.n_win - 1);
  }
  // the tiles that cover the pixels, per axis by the same rule; one pass of both loops unless PLAN is TILES
  int y = 0, x0 = 0, ky_lo = 0, ky_hi = 0, kx_lo = 0, kx_hi = 0;
  if constexpr (PLAN == TILES) {
    y = (int)(p / tg.w);
    x0 = (int)(p % tg.w);
    ky_lo = y < tg.th ? 0 : (y - tg.th) / tg.sy + 1;
    ky_hi = min(y / tg.sy, tg.n_ty - 1);
    kx_lo = x0 < tg.tw ? 0 : (x0 - tg.tw) / tg.sx + 1;
    kx_hi = min(x0 / tg.sx, tg.n_tx - 1);
  }
  for (int kw = k_lo; kw <= k_hi; ++kw) {
    int pos = f;                                                         // position in the window: 0 .. window - 1
    float wgt = 1.f;
    int64_t wrow = bf * hw + p;                                          // eps row of the first pixel
    if constexpr (WINDOWS) {
      pos = f - kw * wp.stride;
      wgt = wn[kw * wp.window + pos];
      wrow = (((int64_t)kw * wp.batch + b) * wp.window + pos) * hw + p;
    }
    float g = 1.f;
    if (eu) g = gs[b * ld_g + pos];                                      // guidance follows the position in the window
    for (int ky = ky_lo; ky <= ky_hi; ++ky)
      for (int kx = kx_lo; kx <= kx_hi; ++kx) {
        float wj[PX];
        int64_t row = wrow;
        if constexpr (PLAN == TILES) {
          const int ly = y - ky * tg.sy, lx = x0 - kx * tg.sx;          // the first pixel inside the tile
#pragma unroll
          for (int j = 0; j < PX; ++j) {
            int lyj = ly, lxj = lx + j;
            while (lxj >= tg.tw) { lxj -= tg.tw; ++lyj; }              // one tile that is the whole frame: into the next row
            wj[j] = (wgt * tg.wy[ky * tg.th + lyj]) * tg.wx[kx * tg.tw + lxj];
          }
          const int64_t patch = ((int64_t)kw * tg.n_ty + ky) * tg.n_tx + kx;
          row = ((patch * wp.batch + b) * wp.window + pos) * ((int64_t)tg.th * tg.tw) + (int64_t)ly * tg.tw + lx;
        } else {
#pragma unroll
          for (int j = 0; j < PX; ++j) wj[j] = wgt;
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
          const f16x4 c4 = *(const f16x4 *)(ec + (row + j) * ld_eps);
          f16x4 u4 = c4;
          if (eu) u4 = *(const f16x4 *)(eu + (row + j) * ld_eps);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float v = eu ? guidance_mix_f16(g, c4[c], u4[c]) : (float)c4[c];
            e[c][j] = WINDOWS ? fmaf(wj[j], v, e[c][j]) : v;             // fp32, never rounded to fp16
          }
        }
      }
  }
  uint64_t seed = 0;
  if constexpr (NOISE) seed = seeds[b];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (NOISE) {
      const int64_t el = ((int64_t)c * frames + f) * hw + p;             // in the video's (4, F_total, H, W) latent
      if constexpr (PX == 4) noise_normals4(noise_block(seed, (uint32_t)(el >> 2), step, NOISE_STEP), z);
      else z[0] = noise_normal_at(seed, el, step, NOISE_STEP);
    }
    vec xo, dn;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      if constexpr (MODE == EULER) {
        xo[j] = NOISE ? euler_ancestral_update(x[c][j], e[c][j], z[j], k) : euler_update(x[c][j], e[c][j], k);
      } else {
        float d;
        xo[j] = (f16)(NOISE ? dpmpp2m_sde_update(x[c][j], e[c][j], dp[c][j], MODE == SECOND_ORDER, z[j], k, &d)
                            : dpmpp2m_update(x[c][j], e[c][j], dp[c][j], MODE == SECOND_ORDER, k, &d));
        dn[j] = (f16)d;
      }
    }
    *(vec *)(out + plane0 + c * cs) = xo;
    if constexpr (MODE != EULER) *(vec *)(out + plane0 + (4 + c) * cs) = dn;
  }
}

// One checked call: the pointers as the entry got them, the constants of its step, its plan (for one set of eps rows: a
// single window that is the whole latent, weights null; for tiles also the space half) and whether the four-pixel form applies.
struct Tail {
  const char *name;
  const f16 *st, *ec, *eu;
  const float *gs, *wn;
  int64_t ld_eps, ld_g, hw;
  f16 *out;
  SamplerCoef k;
  WindowPlan wp;
  TileGeom tg;             // tg.wy != null: the tiles form
  bool wide;
  const uint64_t *seeds;   // [batch] on the device; read only where k.n != 0
  uint32_t step;
};

template <int MODE, bool NOISE>
void launch_form(const Tail &t, void *stream) {
  const int plan = t.tg.wy ? TILES : t.wn ? WINDOWS : ROWS;
  const auto kernel = plan == TILES     ? (t.wide ? sampler_tail_kernel<4, MODE, TILES, NOISE> : sampler_tail_kernel<1, MODE, TILES, NOISE>)
                      : plan == WINDOWS ? (t.wide ? sampler_tail_kernel<4, MODE, WINDOWS, NOISE> : sampler_tail_kernel<1, MODE, WINDOWS, NOISE>)
                                        : (t.wide ? sampler_tail_kernel<4, MODE, ROWS, NOISE> : sampler_tail_kernel<1, MODE, ROWS, NOISE>);
  const int64_t total = (int64_t)t.wp.batch * t.wp.frames * t.hw / (t.wide ? 4 : 1);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t.st, t.ec, t.eu, t.ld_eps,
                     t.gs, t.ld_g, t.wn, t.out, t.k, t.wp, t.tg, t.hw, total, t.seeds, t.step);
}

// n == 0 (the deterministic samplers, eta == 0, the last step) is the kernel without noise: the bytes of the existing entries
template <int MODE>
void launch(const Tail &t, void *stream) {
  if (t.k.n != 0.f) launch_form<MODE, true>(t, stream);
  else launch_form<MODE, false>(t, stream);
}

// The plan of an entry that takes none: the frame windows with their table `wf`, and one tile that is the whole frame.  No
// table is one set of eps rows, which check() holds to one window that is the whole latent; its stride is then the window.
sp_tile_plan frame_plan(int frames_total, int h, int w, int window, int stride, int n_win, const float *wf) {
  return sp_tile_plan{frames_total, window, wf ? stride : window, n_win, h, w, h, w, h, w, 1, 1, wf, nullptr, nullptr};
}

struct Noise {
  float scale;
  const uint64_t *seeds;
  uint32_t step;
};

// Everything the entry points refuse; on success fills the call (but for the step's own constants in t->k).  `tables`: the
// weight tables the entry's form takes, 0 (one set of eps rows), 1 (frame windows: wf) or 3 (tiles: wf, wy, wx).  `noise`:
// the noise arguments of an entry that has them.
int check(const char *name, const sp_tile_plan *pl, int tables, const void *state, const void *eps_cond, const void *eps_uncond,
          int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out, float sigma, int channels, int batch,
          const Noise *noise, Tail *t) {
  SP_REQUIRE(pl, "%s: null plan", name);
  SP_REQUIRE(tables < 3 || (pl->wf && pl->wy && pl->wx),
             "%s: null table (the plan's normalised wf [n_win][window], wy [n_ty][tile_h], wx [n_tx][tile_w])", name);
  SP_REQUIRE(state && eps_cond && out, "%s: null pointer", name);
  SP_REQUIRE(pl->wf || (tables == 0 && pl->n_win == 1 && pl->window == pl->frames_total),
             "%s: null weights (the normalised [n_win][window] table of the window plan)", name);
  SP_REQUIRE(!eps_uncond || guidance, "%s: CFG needs a guidance vector", name);
  SP_REQUIRE(ld_eps >= 4 && ld_eps % 4 == 0, "%s: ld_eps must be a multiple of 4", name);
  SP_REQUIRE(batch > 0 && pl->frames_total > 0 && pl->window > 0 && pl->h > 0 && pl->w > 0 && pl->tile_h > 0 && pl->tile_w > 0,
             "%s: dims must be positive", name);
  // per axis the same rule: 1 <= stride <= tile <= total, the total the tile plus whole strides, n the count that gives
  // (the frames axis is named without the word "stride", so that only the refusals about its stride carry it)
  char frames[64], y[80], x[80];
  snprintf(frames, sizeof(frames), "frames_total=%d, window=%d", pl->frames_total, pl->window);
  snprintf(y, sizeof(y), "y (total, tile, stride) = (%d, %d, %d)", pl->h, pl->tile_h, pl->stride_y);
  snprintf(x, sizeof(x), "x (total, tile, stride) = (%d, %d, %d)", pl->w, pl->tile_w, pl->stride_x);
  const struct { const char *axis, *tile, *stride, *count; int total, t, s, n; } axes[3] = {
      {frames, "window", "stride", "n_win", pl->frames_total, pl->window, pl->stride, pl->n_win},
      {y, "tile", "stride_y", "n_ty", pl->h, pl->tile_h, pl->stride_y, pl->n_ty},
      {x, "tile", "stride_x", "n_tx", pl->w, pl->tile_w, pl->stride_x, pl->n_tx}};
  for (const auto &a : axes) {
    const char *axis = a.axis;
    SP_REQUIRE(a.t <= a.total, "%s: %s: the %s exceeds the total", name, axis, a.tile);
    SP_REQUIRE(a.s >= 1 && a.s <= a.t, "%s: %s: stride must be from 1 to the %s (%s=%d)", name, axis, a.tile, a.stride, a.s);
    SP_REQUIRE((a.total - a.t) % a.s == 0, "%s: %s: the total is not the %s plus a whole number of strides (%s=%d)", name, axis,
               a.tile, a.stride, a.s);
    SP_REQUIRE(a.n == (a.total - a.t) / a.s + 1, "%s: %s=%d, the plan of %s, %d apart, has %d %ss", name, a.count, a.n, axis, a.s,
               (a.total - a.t) / a.s + 1, a.tile);
  }
  SP_REQUIRE(ld_guidance == 0 || ld_guidance >= pl->window,
             "%s: ld_guidance=%lld must be 0 (one shared row) or >= the frames of a window (%d)", name, (long long)ld_guidance,
             pl->window);
  SP_REQUIRE(sigma > 0.f, "%s: sigma must be positive", name);
  const int64_t hw = (int64_t)pl->h * pl->w;
  const int64_t bytes = (int64_t)batch * pl->frames_total * hw * channels * (int64_t)sizeof(f16);
  const uintptr_t s0 = (uintptr_t)state, o0 = (uintptr_t)out;
  SP_REQUIRE(s0 == o0 || s0 + (uintptr_t)bytes <= o0 || o0 + (uintptr_t)bytes <= s0,
             "%s: out must be the input itself or not overlap it", name);
  const float s2 = sigma * sigma + 1.0f;
  // four pixels per thread where every plane access stays 8-byte aligned and the four share a row, their covering tiles and
  // adjacent eps rows inside every tile; one tile that is the whole frame has the frame's pixels in order, across rows too
  const bool wide = hw % 4 == 0 && s0 % 8 == 0 && o0 % 8 == 0 &&
                    ((pl->w % 4 == 0 && pl->tile_w % 4 == 0 && pl->stride_x % 4 == 0) || (pl->n_ty == 1 && pl->n_tx == 1));
  *t = Tail{name, (const f16 *)state, (const f16 *)eps_cond, (const f16 *)eps_uncond, guidance, pl->wf, ld_eps, ld_guidance, hw,
            (f16 *)out, SamplerCoef{-sigma / sqrtf(s2), 1.0f / s2},
            WindowPlan{pl->frames_total, pl->window, pl->stride, pl->n_win, batch},
            TileGeom{pl->w, pl->tile_h, pl->tile_w, pl->stride_y, pl->stride_x, pl->n_ty, pl->n_tx, pl->wy, pl->wx}, wide, nullptr, 0u};
  if (!noise) return SP_OK;
  SP_REQUIRE(noise->scale >= 0.f && noise->scale <= 3.402823466e38f, "%s: noise_scale = %g must be finite and not negative", name,
             (double)noise->scale);
  SP_REQUIRE(noise->scale == 0.f || noise->seeds, "%s: null seeds with noise_scale = %g (one 64-bit seed per video, on the device)",
             name, (double)noise->scale);
  SP_REQUIRE((uintptr_t)noise->seeds % 8 == 0, "%s: seeds must be 8-byte aligned", name);
  SP_REQUIRE(noise_fits(pl->frames_total, hw), "%s: 4*frames_total*h*w = 4*%d*%lld exceeds 2^34, the noise address' range", name,
             pl->frames_total, (long long)hw);
  t->k.n = noise->scale; t->seeds = noise->seeds; t->step = noise->step;
  return SP_OK;
}

// The two updates behind check(): the Euler step to sigma_next (Euler ancestral: to sigma_down) and the 2M step.
int euler_tail(const char *name, const sp_tile_plan *pl, int tables, const void *latent, const void *eps_cond,
               const void *eps_uncond, int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out, float sigma,
               float sigma_next, int batch, const Noise *noise, void *stream) {
  Tail t;
  if (int rc = check(name, pl, tables, latent, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out, sigma, 4, batch, noise, &t))
    return rc;
  t.k.inv_sigma = 1.0f / sigma; t.k.dt = sigma_next - sigma;
  SP_CLEAR_STALE_ERROR();
  launch<EULER>(t, stream);
  SP_CHECK_LAUNCH(name);
  return SP_OK;
}

int dpmpp2m_tail(const char *name, const sp_tile_plan *pl, int tables, const void *state, const void *eps_cond,
                 const void *eps_uncond, int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out_state, float sigma,
                 float a, float b, float c1, float c2, int batch, const Noise *noise, void *stream) {
  Tail t;
  if (int rc = check(name, pl, tables, state, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out_state, sigma, 8, batch, noise,
                     &t))
    return rc;
  SP_REQUIRE(a >= 0.f && a < 1.f, "%s: a = sigma'/sigma = %g must be in [0, 1)", name, (double)a);
  SP_REQUIRE(c2 >= 0.f, "%s: c2 = %g must not be negative", name, (double)c2);
  t.k.a = a; t.k.b = b; t.k.c1 = c1; t.k.c2 = c2;
  SP_CLEAR_STALE_ERROR();
  if (c2 != 0.f) launch<SECOND_ORDER>(t, stream);
  else launch<FIRST_ORDER>(t, stream);
  SP_CHECK_LAUNCH(name);
  return SP_OK;
}

}  // namespace

extern "C" int sp_euler_step_rows_f16(const void *latent, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                      const float *guidance, int64_t ld_guidance, void *out, float sigma, float sigma_next,
                                      int b, int frames, int h, int w, void *stream) {
  const sp_tile_plan pl = frame_plan(frames, h, w, frames, frames, 1, nullptr);
  return euler_tail("sp_euler_step_rows_f16", &pl, 0, latent, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out, sigma,
                    sigma_next, b, nullptr, stream);
}

extern "C" int sp_euler_step_f16(const void *latent, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                 const float *guidance, void *out, float sigma, float sigma_next, int b, int frames, int h,
                                 int w, void *stream) {
  return sp_euler_step_rows_f16(latent, eps_cond, eps_uncond, ld_eps, guidance, 0, out, sigma, sigma_next, b, frames, h, w,
                                stream);
}

extern "C" int sp_dpmpp2m_step_rows_f16(const void *state, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                        const float *guidance, int64_t ld_guidance, void *out_state, float sigma, float a,
                                        float b, float c1, float c2, int batch, int frames, int h, int w, void *stream) {
  const sp_tile_plan pl = frame_plan(frames, h, w, frames, frames, 1, nullptr);
  return dpmpp2m_tail("sp_dpmpp2m_step_rows_f16", &pl, 0, state, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out_state,
                      sigma, a, b, c1, c2, batch, nullptr, stream);
}

extern "C" int sp_euler_step_windows_f16(const void *latent, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                         const float *guidance, int64_t ld_guidance, void *out, float sigma,
                                         float sigma_next, int b, int frames_total, int h, int w, int window, int stride,
                                         int n_win, const float *weights, void *stream) {
  const sp_tile_plan pl = frame_plan(frames_total, h, w, window, stride, n_win, weights);
  return euler_tail("sp_euler_step_windows_f16", &pl, 1, latent, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out, sigma,
                    sigma_next, b, nullptr, stream);
}

extern "C" int sp_dpmpp2m_step_windows_f16(const void *state, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                           const float *guidance, int64_t ld_guidance, void *out_state, float sigma, float a,
                                           float b, float c1, float c2, int batch, int frames_total, int h, int w, int window,
                                           int stride, int n_win, const float *weights, void *stream) {
  const sp_tile_plan pl = frame_plan(frames_total, h, w, window, stride, n_win, weights);
  return dpmpp2m_tail("sp_dpmpp2m_step_windows_f16", &pl, 1, state, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out_state,
                      sigma, a, b, c1, c2, batch, nullptr, stream);
}

extern "C" int sp_euler_ancestral_step_f16(const void *latent, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                           const float *guidance, int64_t ld_guidance, void *out, float sigma,
                                           float sigma_down, int b, int frames_total, int h, int w, int window, int stride,
                                           int n_win, const float *weights, float noise_scale, const uint64_t *seeds,
                                           uint32_t step, void *stream) {
  const sp_tile_plan pl = frame_plan(frames_total, h, w, window, stride, n_win, weights);
  const Noise noise{noise_scale, seeds, step};
  return euler_tail("sp_euler_ancestral_step_f16", &pl, weights ? 1 : 0, latent, eps_cond, eps_uncond, ld_eps, guidance,
                    ld_guidance, out, sigma, sigma_down, b, &noise, stream);
}

extern "C" int sp_dpmpp2m_sde_step_f16(const void *state, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                       const float *guidance, int64_t ld_guidance, void *out_state, float sigma, float a,
                                       float b, float c1, float c2, int batch, int frames_total, int h, int w, int window,
                                       int stride, int n_win, const float *weights, float noise_scale, const uint64_t *seeds,
                                       uint32_t step, void *stream) {
  const sp_tile_plan pl = frame_plan(frames_total, h, w, window, stride, n_win, weights);
  const Noise noise{noise_scale, seeds, step};
  return dpmpp2m_tail("sp_dpmpp2m_sde_step_f16", &pl, weights ? 1 : 0, state, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance,
                      out_state, sigma, a, b, c1, c2, batch, &noise, stream);
}

extern "C" size_t sp_tile_plan_size(void) { return sizeof(sp_tile_plan); }

extern "C" int sp_euler_step_tiles_f16(const sp_tile_plan *plan, const void *latent, const void *eps_cond, const void *eps_uncond,
                                       int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out, float sigma,
                                       float sigma_next_or_down, int batch, float noise_scale, const uint64_t *seeds,
                                       uint32_t step, void *stream) {
  const Noise noise{noise_scale, seeds, step};
  return euler_tail("sp_euler_step_tiles_f16", plan, 3, latent, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out, sigma,
                    sigma_next_or_down, batch, &noise, stream);
}

extern "C" int sp_dpmpp2m_step_tiles_f16(const sp_tile_plan *plan, const void *state, const void *eps_cond, const void *eps_uncond,
                                         int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out_state, float sigma,
                                         float a, float b, float c1, float c2, int batch, float noise_scale,
                                         const uint64_t *seeds, uint32_t step, void *stream) {
  const Noise noise{noise_scale, seeds, step};
  return dpmpp2m_tail("sp_dpmpp2m_step_tiles_f16", plan, 3, state, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out_state,
                      sigma, a, b, c1, c2, batch, &noise, stream);
}
