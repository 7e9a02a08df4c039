// Host-side image handling of the reference's demo, on the device (/root/reference/scripts/generate_video_demo.py:
// load_and_preprocess_image :71-89 = PIL Image.resize(LANCZOS) + crop; encode_image :108-126 = CLIPImageProcessor's
// bicubic resize / crop / normalise and torchvision's ToTensor + Normalize; save_video :198-209 = frames -> uint8).
//
//   resample_axis_kernel : one axis of Pillow's antialiased separable resize on interleaved uint8 RGB.  One thread per
//                          output pixel; the taps and their weights are recomputed per thread (the tap count follows the
//                          reduction factor and is a loop bound).  Geometry in fp64 as Pillow has it, weights and sums
//                          in fp32; the rounded uint8 result is what the second pass reads.
//   copy_rows_kernel     : the pass of an axis whose size does not change.
//   to_tensor_kernel     : uint8 [h][w][3] (any row pitch: a crop is a pointer + pitch) -> fp16 planar (3,h,w),
//                          (v/255 - mean)/std.
//   frames_to_u8_kernel  : video tensor (B,3,F,H,W) fp16 / fp32 -> (B,F,H,W,3) uint8 through frame_level_u8 (common.h),
//                          four pixels per thread: three vector loads along x, one 12-byte store.
// These run once per video on a few MB: none of them is tuned.
#include "common.h"

namespace {

typedef unsigned char u8;
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));

// Pillow's filters (src/libImaging/Resample.c): bicubic with a = -0.5 (support 2), Lanczos with three lobes (support 3)
template <int FILTER>
__device__ __forceinline__ float filter_weight(float x) {
  if (FILTER == SP_FILTER_BICUBIC) {
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
    return 0.0f;
  } else {
    if (x < -3.0f || x >= 3.0f) return 0.0f;
    if (x == 0.0f) return 1.0f;
    const float pi = 3.14159265358979323846f;
    return (sinpif(x) / (pi * x)) * (sinpif(x * (1.0f / 3.0f)) / (pi * x * (1.0f / 3.0f)));
  }
}

// out[y][x] over the axis `horizontal ? x : y`: in_n source samples along that axis -> out_n.  tap k of pixel (y, x) is at
// in + y*in_pitch + k*3 (horizontal) or in + k*in_pitch + x*3 (vertical).
template <int FILTER>
__global__ void resample_axis_kernel(const u8 *__restrict__ in, int64_t in_pitch, u8 *__restrict__ out, int64_t out_pitch,
                                     int out_h, int out_w, int in_n, int out_n, int horizontal, float support_base) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)out_h * out_w) return;
  const int y = (int)(idx / out_w), x = (int)(idx % out_w);
  const int i = horizontal ? x : y;
  const double scale = (double)in_n / (double)out_n;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (double)support_base * fs, inv_fs = 1.0 / fs;
  const double centre = (i + 0.5) * scale;
  int lo = (int)(centre - support + 0.5), hi = (int)(centre + support + 0.5);
  lo = lo < 0 ? 0 : lo;
  hi = hi > in_n ? in_n : hi;
  const u8 *src = horizontal ? in + (int64_t)y * in_pitch : in + (int64_t)x * 3;
  const int64_t step = horizontal ? 3 : in_pitch;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, wsum = 0.f;
  for (int k = lo; k < hi; ++k) {
    const float wgt = filter_weight<FILTER>((float)((k - centre + 0.5) * inv_fs));
    const u8 *p = src + (int64_t)k * step;
    acc0 = fmaf(wgt, (float)p[0], acc0);
    acc1 = fmaf(wgt, (float)p[1], acc1);
    acc2 = fmaf(wgt, (float)p[2], acc2);
    wsum += wgt;
  }
  const float inv = wsum != 0.f ? 1.0f / wsum : 1.0f;
  u8 *dst = out + (int64_t)y * out_pitch + (int64_t)x * 3;
  dst[0] = (u8)(int)fminf(fmaxf(floorf(acc0 * inv + 0.5f), 0.f), 255.f);
  dst[1] = (u8)(int)fminf(fmaxf(floorf(acc1 * inv + 0.5f), 0.f), 255.f);
  dst[2] = (u8)(int)fminf(fmaxf(floorf(acc2 * inv + 0.5f), 0.f), 255.f);
}

__global__ void copy_rows_kernel(const u8 *__restrict__ in, int64_t in_pitch, u8 *__restrict__ out, int64_t out_pitch, int h,
                                 int w) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)h * w) return;
  const int y = (int)(idx / w), x = (int)(idx % w);
  const u8 *p = in + (int64_t)y * in_pitch + (int64_t)x * 3;
  u8 *d = out + (int64_t)y * out_pitch + (int64_t)x * 3;
  d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
}

struct norm3 { float mean[3], std[3]; };

__global__ void to_tensor_kernel(const u8 *__restrict__ in, int64_t pitch, f16 *__restrict__ out, int h, int w, norm3 n) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, hw = (int64_t)h * w;
  if (idx >= hw) return;
  const int y = (int)(idx / w), x = (int)(idx % w);
  const u8 *p = in + (int64_t)y * pitch + (int64_t)x * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c * hw + idx] = (f16)(((float)p[c] / 255.0f - n.mean[c]) / n.std[c]);
}

// one thread per PX consecutive pixels of a frame row-major plane (PX = 4 needs hw % 4 == 0 and aligned pointers)
template <typename IN, int PX>
__global__ void frames_to_u8_kernel(const IN *__restrict__ in, u8 *__restrict__ out, int frames, int64_t hw, int64_t total) {
  const int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PX;     // (b, f, pixel)
  if (idx >= total) return;
  const int64_t p = idx % hw, bf = idx / hw, b = bf / frames, f = bf % frames;
  const IN *src = in + (b * 3 * frames + f) * hw + p;
  if (PX == 4) {
    typedef IN in4 __attribute__((ext_vector_type(4)));
    const in4 r = *(const in4 *)src, g = *(const in4 *)(src + frames * hw), bl = *(const in4 *)(src + 2 * frames * hw);
    u8 v[12];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[3 * e] = frame_level_u8((float)r[e]);
      v[3 * e + 1] = frame_level_u8((float)g[e]);
      v[3 * e + 2] = frame_level_u8((float)bl[e]);
    }
    u32x3 o;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      o[d] = (unsigned)v[4 * d] | ((unsigned)v[4 * d + 1] << 8) | ((unsigned)v[4 * d + 2] << 16) | ((unsigned)v[4 * d + 3] << 24);
    *(u32x3 *)(out + idx * 3) = o;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[idx * 3 + c] = frame_level_u8((float)src[c * frames * hw]);
  }
}

template <int FILTER>
void launch_axis(const u8 *in, int64_t in_pitch, u8 *out, int64_t out_pitch, int out_h, int out_w, int in_n, int out_n,
                 int horizontal, hipStream_t s) {
  const int64_t total = (int64_t)out_h * out_w;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (in_n == out_n)
    hipLaunchKernelGGL(copy_rows_kernel, grid, dim3(256), 0, s, in, in_pitch, out, out_pitch, out_h, out_w);
  else
    hipLaunchKernelGGL(resample_axis_kernel<FILTER>, grid, dim3(256), 0, s, in, in_pitch, out, out_pitch, out_h, out_w, in_n,
                       out_n, horizontal, FILTER == SP_FILTER_BICUBIC ? 2.0f : 3.0f);
}

}  // namespace

extern "C" size_t sp_image_resample_tmp_bytes(int src_h, int dst_w) {
  return src_h > 0 && dst_w > 0 ? (size_t)src_h * (size_t)dst_w * 3 : 0;
}

extern "C" int sp_image_resample_u8(const void *src, int64_t src_pitch, int src_h, int src_w, void *dst, int64_t dst_pitch,
                                    int dst_h, int dst_w, int filter, void *tmp, size_t tmp_bytes, void *stream) {
  SP_REQUIRE(src && dst && tmp, "sp_image_resample_u8: null pointer");
  SP_REQUIRE(src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0, "sp_image_resample_u8: sizes must be positive (%dx%d -> %dx%d)",
             src_h, src_w, dst_h, dst_w);
  SP_REQUIRE(src_pitch >= 3 * (int64_t)src_w && dst_pitch >= 3 * (int64_t)dst_w,
             "sp_image_resample_u8: a row pitch (src %lld, dst %lld bytes) is shorter than 3 * width", (long long)src_pitch,
             (long long)dst_pitch);
  SP_REQUIRE(filter == SP_FILTER_BICUBIC || filter == SP_FILTER_LANCZOS3, "sp_image_resample_u8: unknown filter %d", filter);
  SP_REQUIRE(tmp_bytes >= sp_image_resample_tmp_bytes(src_h, dst_w), "sp_image_resample_u8: tmp holds %zu bytes, needs %zu",
             tmp_bytes, sp_image_resample_tmp_bytes(src_h, dst_w));
  SP_REQUIRE(((int64_t)src_h * dst_w + 255) / 256 <= 0x7fffffff && ((int64_t)dst_h * dst_w + 255) / 256 <= 0x7fffffff,
             "sp_image_resample_u8: too many pixels");
  hipStream_t s = (hipStream_t)stream;
  const int64_t tmp_pitch = 3 * (int64_t)dst_w;
  SP_CLEAR_STALE_ERROR();
  if (filter == SP_FILTER_BICUBIC) {
    launch_axis<SP_FILTER_BICUBIC>((const u8 *)src, src_pitch, (u8 *)tmp, tmp_pitch, src_h, dst_w, src_w, dst_w, 1, s);
    launch_axis<SP_FILTER_BICUBIC>((const u8 *)tmp, tmp_pitch, (u8 *)dst, dst_pitch, dst_h, dst_w, src_h, dst_h, 0, s);
  } else {
    launch_axis<SP_FILTER_LANCZOS3>((const u8 *)src, src_pitch, (u8 *)tmp, tmp_pitch, src_h, dst_w, src_w, dst_w, 1, s);
    launch_axis<SP_FILTER_LANCZOS3>((const u8 *)tmp, tmp_pitch, (u8 *)dst, dst_pitch, dst_h, dst_w, src_h, dst_h, 0, s);
  }
  SP_CHECK_LAUNCH("sp_image_resample_u8");
  return SP_OK;
}

extern "C" int sp_image_to_tensor_f16(const void *src, int64_t src_pitch, int h, int w, void *out, float mean0, float mean1,
                                      float mean2, float std0, float std1, float std2, void *stream) {
  SP_REQUIRE(src && out, "sp_image_to_tensor_f16: null pointer");
  SP_REQUIRE(h > 0 && w > 0, "sp_image_to_tensor_f16: sizes must be positive (%dx%d)", h, w);
  SP_REQUIRE(src_pitch >= 3 * (int64_t)w, "sp_image_to_tensor_f16: row pitch %lld bytes is shorter than 3 * width",
             (long long)src_pitch);
  SP_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "sp_image_to_tensor_f16: std must not be zero");
  const int64_t total = (int64_t)h * w;
  SP_REQUIRE((total + 255) / 256 <= 0x7fffffff, "sp_image_to_tensor_f16: too many pixels");
  const norm3 n = {{mean0, mean1, mean2}, {std0, std1, std2}};
  SP_CLEAR_STALE_ERROR();
  hipLaunchKernelGGL(to_tensor_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u8 *)src,
                     src_pitch, (f16 *)out, h, w, n);
  SP_CHECK_LAUNCH("sp_image_to_tensor_f16");
  return SP_OK;
}

extern "C" int sp_frames_to_u8(const void *frames, int is_fp32, void *out, int batch, int frames_n, int h, int w, void *stream) {
  SP_REQUIRE(frames && out, "sp_frames_to_u8: null pointer");
  SP_REQUIRE(batch > 0 && frames_n > 0 && h > 0 && w > 0, "sp_frames_to_u8: sizes must be positive");
  const int64_t hw = (int64_t)h * w, total = (int64_t)batch * frames_n * hw;
  SP_REQUIRE((total + 255) / 256 <= 0x7fffffff, "sp_frames_to_u8: too many pixels");
  hipStream_t s = (hipStream_t)stream;
  // four pixels per thread where a group of four never leaves its plane and the vector accesses are aligned
  const bool vec = hw % 4 == 0 && (uintptr_t)frames % (is_fp32 ? 16 : 8) == 0 && (uintptr_t)out % 4 == 0;
  const dim3 grid((unsigned)(((vec ? total / 4 : total) + 255) / 256));
  SP_CLEAR_STALE_ERROR();
#define SP_LAUNCH_FRAMES_TO_U8(IN, PX) \
  hipLaunchKernelGGL((frames_to_u8_kernel<IN, PX>), grid, dim3(256), 0, s, (const IN *)frames, (u8 *)out, frames_n, hw, total)
  if (is_fp32) {
    if (vec) SP_LAUNCH_FRAMES_TO_U8(float, 4);
    else SP_LAUNCH_FRAMES_TO_U8(float, 1);
  } else {
    if (vec) SP_LAUNCH_FRAMES_TO_U8(f16, 4);
    else SP_LAUNCH_FRAMES_TO_U8(f16, 1);
  }
#undef SP_LAUNCH_FRAMES_TO_U8
  SP_CHECK_LAUNCH("sp_frames_to_u8");
  return SP_OK;
}
