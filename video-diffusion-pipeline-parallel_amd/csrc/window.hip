// Sampler tails behind overlapping frame windows (temporal co-denoising): a latent of F_total frames is cut into n_win windows
// of `window` frames, `stride` apart; the UNet ran once per window and left each window's eps rows in one buffer
// [n_win][B][window][H*W][ld_eps].  These kernels blend the windows' predictions frame by frame with the host's normalised
// weight table and apply ONE sampler update to the whole latent: the Euler update of euler_kernel (elementwise.hip) or the
// DPM-Solver++(2M) update of dpmpp2m_kernel (solver.hip), expression for expression, with the fused fp32 eps in place of the
// single window's.  See sp_euler_step_windows_f16 / sp_dpmpp2m_step_windows_f16 in svdpipe.h.
#include "common.h"

namespace {

struct WindowPlan {
  int frames, window, stride, n_win, batch;   // frames = F_total
};

struct Coef {
  float c_out, c_skip;
  float inv_sigma, dt;      // Euler
  float a, b, c1, c2;       // 2M
};

// a*b + c rounded to fp16 inside the fma.  euler_kernel stores scalars, for which the compiler fuses the final fma with the
// conversion into this instruction; for the packed stores of PX = 4 it would emit an fp32 fma and a packed conversion, which
// rounds twice and gives other bytes.  The Euler form below asks for the instruction, so that both PX agree with euler_kernel.
__device__ __forceinline__ f16 fma_to_f16(float a, float b, float c) {
  f16 r;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

enum { EULER = 0, FIRST_ORDER = 1, SECOND_ORDER = 2 };   // FIRST_ORDER: 2M with c2 == 0, the D_prev planes are never read

// A thread owns PX adjacent pixels of one (b, f) of the long latent, as in dpmpp2m_kernel: the planes are read and written PX
// at a time (8 bytes for PX = 4), the eps rows one 8-byte row per pixel and covering window.  Every value a thread reads from
// `st` is in a register before its first store and no other thread touches those elements, so out == st is safe; hence no
// __restrict__ on the two.
template <int PX, int MODE>
__global__ __launch_bounds__(256) void window_step_kernel(const f16 *st, const f16 *__restrict__ ec,
                                                          const f16 *__restrict__ eu, int64_t ld_eps,
                                                          const float *__restrict__ gs, int64_t ld_g,
                                                          const float *__restrict__ wn, f16 *out, Coef k, WindowPlan wp,
                                                          int64_t hw, int64_t total) {
  typedef f16 vec __attribute__((ext_vector_type(PX)));
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
      if (MODE == SECOND_ORDER) dp[c][0] = (float)st[plane0 + (4 + c) * cs];
    } else {
      const vec xv = *(const vec *)(st + plane0 + c * cs);
#pragma unroll
      for (int j = 0; j < PX; ++j) x[c][j] = (float)xv[j];
      if (MODE == SECOND_ORDER) {
        const vec dv = *(const vec *)(st + plane0 + (4 + c) * cs);
#pragma unroll
        for (int j = 0; j < PX; ++j) dp[c][j] = (float)dv[j];
      }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) e[c][j] = 0.f;
  }
  // the windows that cover global frame f, in ascending order: k*stride <= f <= k*stride + window - 1
  const int k_lo = f < wp.window ? 0 : (f - wp.window) / wp.stride + 1;
  const int k_hi = min(f / wp.stride, wp.n_win - 1);
  for (int kw = k_lo; kw <= k_hi; ++kw) {
    const int pos = f - kw * wp.stride;                                  // position in the window: 0 .. window - 1
    const float wgt = wn[kw * wp.window + pos];
    const int64_t row = (((int64_t)kw * wp.batch + b) * wp.window + pos) * hw + p;   // eps row of the first pixel
    float g = 1.f;
    if (eu) g = gs[b * ld_g + pos];                                      // guidance follows the position in the window
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const f16x4 c4 = *(const f16x4 *)(ec + (row + j) * ld_eps);
      f16x4 u4 = c4;
      if (eu) u4 = *(const f16x4 *)(eu + (row + j) * ld_eps);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float v = (float)c4[c];
        if (eu) {
          // the guidance mix in fp16, rounding for rounding as euler_kernel (reference svd_unet.py:410-411)
          const f16 gh = (f16)g;
          const f16 diff = (f16)((float)c4[c] - (float)u4[c]);
          const f16 prod = (f16)((float)gh * (float)diff);
          v = (float)(f16)((float)u4[c] + (float)prod);
        }
        e[c][j] = fmaf(wgt, v, e[c][j]);                                 // fp32, never rounded to fp16
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    vec xo, dn;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      float xn, d;
      if constexpr (MODE == EULER) {
        // the expression of euler_kernel as the compiler contracts it there (e*c_out + x*c_skip: the first product joins the
        // sum; left to itself it pairs the two products of PX = 4 into a packed multiply and adds); x + d*dt leaves as fp16
        const float x0 = fmaf(e[c][j], k.c_out, x[c][j] * k.c_skip);
        d = (x[c][j] - x0) * k.inv_sigma;
        const f16 xh = fma_to_f16(k.dt, d, x[c][j]);
        if constexpr (PX == 1) out[plane0 + c * cs] = xh;
        else xo[j] = xh;
        continue;
      } else {
        // the expressions of dpmpp2m_kernel
        d = fmaf(x[c][j], k.c_skip, e[c][j] * k.c_out);
        const float dd = MODE == SECOND_ORDER ? fmaf(k.c1, d, -(k.c2 * dp[c][j])) : d;
        xn = fmaf(k.a, x[c][j], k.b * dd);
      }
      if constexpr (PX == 1) {
        out[plane0 + c * cs] = (f16)xn;
        out[plane0 + (4 + c) * cs] = (f16)d;
      } else {
        xo[j] = (f16)xn;
        dn[j] = (f16)d;
      }
    }
    if constexpr (PX > 1) {
      *(vec *)(out + plane0 + c * cs) = xo;
      if (MODE != EULER) *(vec *)(out + plane0 + (4 + c) * cs) = dn;
    }
  }
}

template <int PX, int MODE>
void launch(int64_t total, hipStream_t s, const f16 *st, const f16 *ec, const f16 *eu, int64_t ld_eps, const float *gs,
            int64_t ld_g, const float *wn, f16 *out, const Coef &k, const WindowPlan &wp, int64_t hw) {
  hipLaunchKernelGGL((window_step_kernel<PX, MODE>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st, ec, eu,
                     ld_eps, gs, ld_g, wn, out, k, wp, hw, total);
}

// Everything both entry points refuse; on success fills the plan and says whether the four-pixel form applies.
int check(const char *name, const void *state, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
          const float *guidance, int64_t ld_guidance, void *out, float sigma, int channels, int batch, int frames_total,
          int window, int stride, int n_win, const float *weights, int h, int w, WindowPlan *wp, bool *wide) {
  SP_REQUIRE(state && eps_cond && out, "%s: null pointer", name);
  SP_REQUIRE(weights, "%s: null weights (the normalised [n_win][window] table of the window plan)", name);
  SP_REQUIRE(!eps_uncond || guidance, "%s: CFG needs a guidance vector", name);
  SP_REQUIRE(ld_eps >= 4 && ld_eps % 4 == 0, "%s: ld_eps must be a multiple of 4", name);
  SP_REQUIRE(batch > 0 && frames_total > 0 && window > 0 && h > 0 && w > 0, "%s: dims must be positive", name);
  SP_REQUIRE(window <= frames_total, "%s: window=%d exceeds frames_total=%d", name, window, frames_total);
  SP_REQUIRE(stride >= 1 && stride <= window, "%s: stride=%d must be from 1 to window (%d)", name, stride, window);
  SP_REQUIRE((frames_total - window) % stride == 0,
             "%s: frames_total=%d is not window (%d) plus a whole number of strides (%d)", name, frames_total, window, stride);
  SP_REQUIRE(n_win == (frames_total - window) / stride + 1, "%s: n_win=%d, the plan of (%d, %d, %d) has %d windows", name,
             n_win, frames_total, window, stride, (frames_total - window) / stride + 1);
  SP_REQUIRE(ld_guidance == 0 || ld_guidance >= window,
             "%s: ld_guidance=%lld must be 0 (one shared row) or >= window (%d)", name, (long long)ld_guidance, window);
  SP_REQUIRE(sigma > 0.f, "%s: sigma must be positive", name);
  const int64_t hw = (int64_t)h * w;
  const int64_t bytes = (int64_t)batch * frames_total * hw * channels * (int64_t)sizeof(f16);
  const uintptr_t s0 = (uintptr_t)state, o0 = (uintptr_t)out;
  SP_REQUIRE(s0 == o0 || s0 + (uintptr_t)bytes <= o0 || o0 + (uintptr_t)bytes <= s0,
             "%s: out must be the input itself or not overlap it", name);
  *wp = WindowPlan{frames_total, window, stride, n_win, batch};
  // four pixels per thread where every plane access stays 8-byte aligned
  *wide = hw % 4 == 0 && s0 % 8 == 0 && o0 % 8 == 0;
  return SP_OK;
}

}  // namespace

extern "C" int sp_euler_step_windows_f16(const void *latent, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                         const float *guidance, int64_t ld_guidance, void *out, float sigma,
                                         float sigma_next, int b, int frames_total, int h, int w, int window, int stride,
                                         int n_win, const float *weights, void *stream) {
  static const char *name = "sp_euler_step_windows_f16";
  WindowPlan wp;
  bool wide;
  if (int rc = check(name, latent, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out, sigma, 4, b, frames_total,
                     window, stride, n_win, weights, h, w, &wp, &wide))
    return rc;
  const int64_t hw = (int64_t)h * w, pixels = (int64_t)b * frames_total * hw;
  const float s2 = sigma * sigma + 1.0f;
  Coef k{};
  k.c_out = -sigma / sqrtf(s2); k.c_skip = 1.0f / s2; k.inv_sigma = 1.0f / sigma; k.dt = sigma_next - sigma;
  SP_CLEAR_STALE_ERROR();
  if (wide)
    launch<4, EULER>(pixels / 4, (hipStream_t)stream, (const f16 *)latent, (const f16 *)eps_cond, (const f16 *)eps_uncond,
                     ld_eps, guidance, ld_guidance, weights, (f16 *)out, k, wp, hw);
  else
    launch<1, EULER>(pixels, (hipStream_t)stream, (const f16 *)latent, (const f16 *)eps_cond, (const f16 *)eps_uncond, ld_eps,
                     guidance, ld_guidance, weights, (f16 *)out, k, wp, hw);
  SP_CHECK_LAUNCH(name);
  return SP_OK;
}

extern "C" int sp_dpmpp2m_step_windows_f16(const void *state, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                           const float *guidance, int64_t ld_guidance, void *out_state, float sigma, float a,
                                           float b, float c1, float c2, int batch, int frames_total, int h, int w, int window,
                                           int stride, int n_win, const float *weights, void *stream) {
  static const char *name = "sp_dpmpp2m_step_windows_f16";
  WindowPlan wp;
  bool wide;
  if (int rc = check(name, state, eps_cond, eps_uncond, ld_eps, guidance, ld_guidance, out_state, sigma, 8, batch,
                     frames_total, window, stride, n_win, weights, h, w, &wp, &wide))
    return rc;
  SP_REQUIRE(a >= 0.f && a < 1.f, "%s: a = sigma'/sigma = %g must be in [0, 1)", name, (double)a);
  SP_REQUIRE(c2 >= 0.f, "%s: c2 = %g must not be negative", name, (double)c2);
  const int64_t hw = (int64_t)h * w, pixels = (int64_t)batch * frames_total * hw;
  const float s2 = sigma * sigma + 1.0f;
  Coef k{};
  k.c_out = -sigma / sqrtf(s2); k.c_skip = 1.0f / s2; k.a = a; k.b = b; k.c1 = c1; k.c2 = c2;
  const f16 *st = (const f16 *)state, *ec = (const f16 *)eps_cond, *eu = (const f16 *)eps_uncond;
  hipStream_t s = (hipStream_t)stream;
  SP_CLEAR_STALE_ERROR();
  if (wide && c2 != 0.f)
    launch<4, SECOND_ORDER>(pixels / 4, s, st, ec, eu, ld_eps, guidance, ld_guidance, weights, (f16 *)out_state, k, wp, hw);
  else if (wide)
    launch<4, FIRST_ORDER>(pixels / 4, s, st, ec, eu, ld_eps, guidance, ld_guidance, weights, (f16 *)out_state, k, wp, hw);
  else if (c2 != 0.f)
    launch<1, SECOND_ORDER>(pixels, s, st, ec, eu, ld_eps, guidance, ld_guidance, weights, (f16 *)out_state, k, wp, hw);
  else
    launch<1, FIRST_ORDER>(pixels, s, st, ec, eu, ld_eps, guidance, ld_guidance, weights, (f16 *)out_state, k, wp, hw);
  SP_CHECK_LAUNCH(name);
  return SP_OK;
}
