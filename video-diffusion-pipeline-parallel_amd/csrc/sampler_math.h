// The arithmetic of the sampler tails, stated once: the fp16 guidance mix, the Euler update and the DPM-Solver++(2M) update of
// one latent value, and the two stochastic forms that add n*z behind them.  sampler_tail.hip evaluates every tail with these
// functions; the conv_out epilogue of gemm.hip keeps a copy of the mix and the Euler update in plain C that must return the same
// bytes
// (tests/test_unet_gpu.py::test_euler_tail_in_conv_out_epilogue_is_bit_identical).
//
// Every body is compiled with fp contraction off and names each fused operation as an fmaf, so where a product is rounded
// on its own and where it joins a sum is written here and not left to the compiler: left alone it contracts the mix's fp16
// multiply and add (two roundings, as the reference has) into one v_fma_f16 in some callers and not in others.
#pragma once
#include "common.h"

// The constants of one step: c_out and c_skip of the v-prediction, then the Euler pair or the 2M coefficients.
struct SamplerCoef {
  float c_out, c_skip;
  float inv_sigma, dt;      // Euler
  float a, b, c1, c2;       // 2M
  float n;                  // noise scale of the step (Euler ancestral, 2M SDE); 0 in the deterministic samplers
};

// a*b + c rounded to fp16 inside the fma.  For a scalar store the compiler fuses an fp32 fma with the conversion behind it
// into this instruction; for the packed stores of four pixels per thread it emits an fp32 fma and a packed conversion, which
// rounds twice and gives other bytes.  The Euler update asks for the instruction, so that every form agrees.
__device__ __forceinline__ f16 fma_to_f16(float a, float b, float c) {
  f16 r;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// eps_u + g*(eps_c - eps_u) in fp16, rounding for rounding as the reference evaluates it on fp16 tensors (svd_unet.py:410-411):
// the scale, the difference, the product and the sum are each rounded to fp16.
__device__ __forceinline__ float guidance_mix_f16(float g, f16 c, f16 u) {
#pragma clang fp contract(off)
  const f16 gh = (f16)g;
  const f16 diff = (f16)((float)c - (float)u);
  const f16 prod = (f16)((float)gh * (float)diff);
  return (float)(f16)((float)u + (float)prod);
}

// x + (x - x0)/sigma * (sigma' - sigma) with x0 = c_skip*x + c_out*e: the product with e joins the sum, the one with x is
// rounded first; the new value is rounded once, to fp16.
__device__ __forceinline__ f16 euler_update(float x, float e, const SamplerCoef &k) {
#pragma clang fp contract(off)
  const float x0 = fmaf(e, k.c_out, x * k.c_skip);
  const float d = (x - x0) * k.inv_sigma;
  return fma_to_f16(k.dt, d, x);
}

// D = c_skip*x + c_out*e and x' = a*x + b*(c1*D - c2*D_prev); without history (c2 == 0, c1 == 1) the bracket is D and
// d_prev is not looked at.  Both leave in fp32.
__device__ __forceinline__ float dpmpp2m_update(float x, float e, float d_prev, bool history, const SamplerCoef &k,
                                                float *denoised) {
#pragma clang fp contract(off)
  const float d = fmaf(x, k.c_skip, e * k.c_out);
  const float dd = history ? fmaf(k.c1, d, -(k.c2 * d_prev)) : d;
  *denoised = d;
  return fmaf(k.a, x, k.b * dd);
}

// The Euler ancestral step: the Euler update towards sigma_down (k.dt = sigma_down - sigma) kept in fp32, t = dt*d + x, and
// the step's noise joins it inside the one rounding to fp16: n*z + t.
__device__ __forceinline__ f16 euler_ancestral_update(float x, float e, float z, const SamplerCoef &k) {
#pragma clang fp contract(off)
  const float x0 = fmaf(e, k.c_out, x * k.c_skip);
  const float d = (x - x0) * k.inv_sigma;
  const float t = fmaf(k.dt, d, x);
  return fma_to_f16(k.n, z, t);
}

// The 2M SDE step: x' = n*z + (a*x + b*(c1*D - c2*D_prev)), the deterministic update as dpmpp2m_update rounds it and one more
// fma; D leaves without noise.  Both in fp32.
__device__ __forceinline__ float dpmpp2m_sde_update(float x, float e, float d_prev, bool history, float z, const SamplerCoef &k,
                                                    float *denoised) {
#pragma clang fp contract(off)
  const float d = fmaf(x, k.c_skip, e * k.c_out);
  const float dd = history ? fmaf(k.c1, d, -(k.c2 * d_prev)) : d;
  *denoised = d;
  return fmaf(k.n, z, fmaf(k.a, x, k.b * dd));
}
