// DPM-Solver++(2M) update behind the UNet's eps rows: the multistep counterpart of euler_kernel (elementwise.hip).
// The solver's history, the previous step's denoised estimate, rides in the latent itself: the carried tensor is
// (B,8,F,H,W), channels 0-3 the sample x, channels 4-7 D_prev.  See sp_dpmpp2m_step_rows_f16 in svdpipe.h.
#include "common.h"

namespace {

// A thread owns PX adjacent pixels of one (b, f): the eight planes are read and written PX at a time (8 bytes for PX = 4),
// the eps rows one 8-byte row per pixel.  Every value a thread reads from `st` is in a register before its first store and
// no other thread touches those elements, so out == st (update in place) is safe; hence no __restrict__ on the two.
// HIST = false (c2 == 0: the first and the last step): the D_prev planes are never read.
template <int PX, bool HIST>
__global__ __launch_bounds__(256) void dpmpp2m_kernel(const f16 *st, const f16 *__restrict__ ec,
                                                      const f16 *__restrict__ eu, int64_t ld_eps,
                                                      const float *__restrict__ gs, int64_t ld_g, f16 *out, float c_out,
                                                      float c_skip, float a, float b_, float c1, float c2, int frames,
                                                      int64_t hw, int64_t total) {
  typedef f16 vec __attribute__((ext_vector_type(PX)));
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one group of PX pixels of a (b, f)
  if (idx >= total) return;
  const int64_t groups = hw / PX;
  const int64_t p = (idx % groups) * PX;
  const int64_t bf = idx / groups;
  const int f = (int)(bf % frames);
  const int64_t b = bf / frames;
  const int64_t row = bf * hw + p;                                       // eps row of the first pixel
  const int64_t plane0 = (b * 8 * frames + f) * hw + p;                  // channel c: + c * frames * hw
  const int64_t cs = (int64_t)frames * hw;

  float x[4][PX], dp[4][PX], e[4][PX];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if constexpr (PX == 1) {
      x[c][0] = (float)st[plane0 + c * cs];
      if (HIST) dp[c][0] = (float)st[plane0 + (4 + c) * cs];
    } else {
      const vec xv = *(const vec *)(st + plane0 + c * cs);
#pragma unroll
      for (int j = 0; j < PX; ++j) x[c][j] = (float)xv[j];
      if (HIST) {
        const vec dv = *(const vec *)(st + plane0 + (4 + c) * cs);
#pragma unroll
        for (int j = 0; j < PX; ++j) dp[c][j] = (float)dv[j];
      }
    }
  }
  float g = 1.f;
  if (eu) g = gs[b * ld_g + f];
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
      e[c][j] = v;
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    vec xo, dn;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float d = fmaf(x[c][j], c_skip, e[c][j] * c_out);           // v-prediction: c_skip and c_out of euler_kernel
      const float dd = HIST ? fmaf(c1, d, -(c2 * dp[c][j])) : d;         // (c1 == 1 where c2 == 0)
      const float xn = fmaf(a, x[c][j], b_ * dd);
      if constexpr (PX == 1) { out[plane0 + c * cs] = (f16)xn; out[plane0 + (4 + c) * cs] = (f16)d; }
      else { xo[j] = (f16)xn; dn[j] = (f16)d; }
    }
    if constexpr (PX > 1) {
      *(vec *)(out + plane0 + c * cs) = xo;
      *(vec *)(out + plane0 + (4 + c) * cs) = dn;
    }
  }
}

template <int PX>
void launch(bool hist, int64_t total, hipStream_t s, const f16 *st, const f16 *ec, const f16 *eu, int64_t ld_eps,
            const float *gs, int64_t ld_g, f16 *out, float c_out, float c_skip, float a, float b, float c1, float c2,
            int frames, int64_t hw) {
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (hist)
    hipLaunchKernelGGL((dpmpp2m_kernel<PX, true>), grid, block, 0, s, st, ec, eu, ld_eps, gs, ld_g, out, c_out, c_skip, a, b,
                       c1, c2, frames, hw, total);
  else
    hipLaunchKernelGGL((dpmpp2m_kernel<PX, false>), grid, block, 0, s, st, ec, eu, ld_eps, gs, ld_g, out, c_out, c_skip, a, b,
                       c1, c2, frames, hw, total);
}

}  // namespace

extern "C" int sp_dpmpp2m_step_rows_f16(const void *state, const void *eps_cond, const void *eps_uncond, int64_t ld_eps,
                                        const float *guidance, int64_t ld_guidance, void *out_state, float sigma, float a,
                                        float b, float c1, float c2, int batch, int frames, int h, int w, void *stream) {
  SP_REQUIRE(state && eps_cond && out_state, "sp_dpmpp2m_step_rows_f16: null pointer");
  SP_REQUIRE(!eps_uncond || guidance, "sp_dpmpp2m_step_rows_f16: CFG needs a guidance vector");
  SP_REQUIRE(ld_eps >= 4 && ld_eps % 4 == 0, "sp_dpmpp2m_step_rows_f16: ld_eps must be a multiple of 4");
  SP_REQUIRE(batch > 0 && frames > 0 && h > 0 && w > 0, "sp_dpmpp2m_step_rows_f16: dims must be positive");
  SP_REQUIRE(ld_guidance == 0 || ld_guidance >= frames,
             "sp_dpmpp2m_step_rows_f16: ld_guidance=%lld must be 0 (one shared row) or >= frames (%d)",
             (long long)ld_guidance, frames);
  SP_REQUIRE(sigma > 0.f, "sp_dpmpp2m_step_rows_f16: sigma must be positive");
  SP_REQUIRE(a >= 0.f && a < 1.f, "sp_dpmpp2m_step_rows_f16: a = sigma'/sigma = %g must be in [0, 1)", (double)a);
  SP_REQUIRE(c2 >= 0.f, "sp_dpmpp2m_step_rows_f16: c2 = %g must not be negative", (double)c2);
  const int64_t hw = (int64_t)h * w, pixels = (int64_t)batch * frames * hw;
  const int64_t bytes = pixels * 8 * (int64_t)sizeof(f16);
  const uintptr_t s0 = (uintptr_t)state, o0 = (uintptr_t)out_state;
  SP_REQUIRE(s0 == o0 || s0 + (uintptr_t)bytes <= o0 || o0 + (uintptr_t)bytes <= s0,
             "sp_dpmpp2m_step_rows_f16: out_state must be state itself or not overlap it");
  // four pixels per thread where every plane access stays 8-byte aligned
  const bool wide = hw % 4 == 0 && s0 % 8 == 0 && o0 % 8 == 0;
  const float s2 = sigma * sigma + 1.0f;
  const float c_out = -sigma / sqrtf(s2), c_skip = 1.0f / s2;
  SP_CLEAR_STALE_ERROR();
  if (wide)
    launch<4>(c2 != 0.f, pixels / 4, (hipStream_t)stream, (const f16 *)state, (const f16 *)eps_cond,
              (const f16 *)eps_uncond, ld_eps, guidance, ld_guidance, (f16 *)out_state, c_out, c_skip, a, b, c1, c2, frames, hw);
  else
    launch<1>(c2 != 0.f, pixels, (hipStream_t)stream, (const f16 *)state, (const f16 *)eps_cond, (const f16 *)eps_uncond,
              ld_eps, guidance, ld_guidance, (f16 *)out_state, c_out, c_skip, a, b, c1, c2, frames, hw);
  SP_CHECK_LAUNCH("sp_dpmpp2m_step_rows_f16");
  return SP_OK;
}
