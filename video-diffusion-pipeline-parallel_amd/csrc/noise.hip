// The generator of noise.h written out: sp_randn_f16, the initial latent of the device noise route (and, with purpose 1, the
// normals a sampler tail adds at a step), and sp_philox_blocks_u32, the raw words for the exact test.  One thread per block of
// four values; a video's latent (4, F, H, W) is 4*F*H*W values, always whole blocks.
#include "noise.h"
#include "sampler_math.h"

namespace {

// out (B, 4, F, H, W) fp16, per_video = F*H*W blocks of each video.  WIDE: every block of four values is 8-byte aligned.
template <bool WIDE>
__global__ __launch_bounds__(256) void randn_kernel(f16 *out, const uint64_t *__restrict__ seeds, float scale,
                                                    int64_t per_video, int64_t total, uint32_t step, uint32_t purpose) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / per_video, j = idx % per_video;
  float z[4];
  noise_normals4(noise_block(seeds[b], (uint32_t)j, step, purpose), z);
  // scale*z rounded ONCE, to fp16, in both forms (sampler_math.h: left to the compiler, a scalar store gets the fused
  // instruction and a packed one a product and a conversion, which round twice); it is what a tail stores for x = 0, n = scale
  f16x4 v;
#pragma unroll
  for (int l = 0; l < 4; ++l) v[l] = fma_to_f16(scale, z[l], 0.0f);
  f16 *dst = out + idx * 4;
  if constexpr (WIDE) {
    *(f16x4 *)dst = v;
  } else {
#pragma unroll
    for (int l = 0; l < 4; ++l) dst[l] = v[l];
  }
}

__global__ __launch_bounds__(256) void philox_blocks_kernel(uint32_t *out, const uint64_t *__restrict__ seeds, int64_t n_blocks,
                                                            int64_t total, uint32_t step, uint32_t purpose) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const PhiloxBlock blk = noise_block(seeds[idx / n_blocks], (uint32_t)(idx % n_blocks), step, purpose);
  *(uint4 *)(out + idx * 4) = make_uint4(blk.u[0], blk.u[1], blk.u[2], blk.u[3]);
}

}  // namespace

extern "C" int sp_randn_f16(void *out, const uint64_t *seeds, float scale, int batch, int frames, int h, int w, uint32_t step,
                            uint32_t purpose, void *stream) {
  const char *name = "sp_randn_f16";
  SP_REQUIRE(out && seeds, "%s: null pointer", name);
  SP_REQUIRE((uintptr_t)out % 2 == 0 && (uintptr_t)seeds % 8 == 0, "%s: out must be 2-byte, seeds 8-byte aligned", name);
  SP_REQUIRE(batch > 0 && frames > 0 && h > 0 && w > 0, "%s: dims must be positive", name);
  SP_REQUIRE(scale >= 0.f && scale <= 3.402823466e38f, "%s: scale = %g must be finite and not negative", name, (double)scale);
  const int64_t hw = (int64_t)h * w;
  SP_REQUIRE(noise_fits(frames, hw), "%s: 4*frames*h*w = 4*%d*%lld exceeds 2^34, the noise address' range", name, frames,
             (long long)hw);
  const int64_t per_video = (int64_t)frames * hw, total = per_video * batch;
  SP_REQUIRE(total <= (int64_t)0x7fffffff * 256, "%s: batch*frames*h*w = %lld is more than one grid", name, (long long)total);
  const dim3 grid((unsigned)((total + 255) / 256));
  SP_CLEAR_STALE_ERROR();
  if ((uintptr_t)out % 8 == 0)
    hipLaunchKernelGGL(randn_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (f16 *)out, seeds, scale, per_video, total, step,
                       purpose);
  else
    hipLaunchKernelGGL(randn_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (f16 *)out, seeds, scale, per_video, total, step,
                       purpose);
  SP_CHECK_LAUNCH(name);
  return SP_OK;
}

extern "C" int sp_philox_blocks_u32(uint32_t *out, const uint64_t *seeds, int batch, int64_t n_blocks, uint32_t step,
                                    uint32_t purpose, void *stream) {
  const char *name = "sp_philox_blocks_u32";
  SP_REQUIRE(out && seeds, "%s: null pointer", name);
  SP_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)seeds % 8 == 0, "%s: out must be 16-byte, seeds 8-byte aligned", name);
  SP_REQUIRE(batch > 0 && n_blocks > 0, "%s: dims must be positive", name);
  SP_REQUIRE(n_blocks <= ((int64_t)1 << 32), "%s: n_blocks = %lld exceeds 2^32, the block counter's range", name,
             (long long)n_blocks);
  SP_REQUIRE(n_blocks <= (int64_t)0x7fffffff * 256 / batch, "%s: batch*n_blocks is more than one grid", name);
  const int64_t total = n_blocks * batch;
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(philox_blocks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, seeds,
                     n_blocks, total, step, purpose);
  SP_CHECK_LAUNCH(name);
  return SP_OK;
}
