// The noise of the stochastic samplers, device-only: a counter-based generator (Philox4x32-10, the Random123 / cuRAND
// construction) and the Box-Muller normals behind it.  A value is a pure function of (the video's 64-bit seed, the step, the
// purpose, the element's position in the video's latent): no state, nothing stored, nothing that depends on the video's row in
// the batch, on the windows or on the rank.  sampler_tail.hip evaluates it in registers, noise.hip writes it out
// (sp_randn_f16, sp_philox_blocks_u32).  DESIGN.md section 18.
//
// Address: element (c, f, p) of a video's latent (4, F_total, H, W) has the flat index e = (c*F_total + f)*H*W + p; block
// j = e >> 2, lane l = e & 3; counter (j, step, purpose, 0); key (seed & 0xffffffff, seed >> 32).  4*F_total*H*W <= 2^34 keeps
// j in 32 bits (noise_fits).
#pragma once
#include "common.h"

enum { NOISE_INITIAL = 0, NOISE_STEP = 1 };   // `purpose`: the initial latent (step 0), the sampler's per-step noise

// the largest latent of one video the address covers: 4*F_total*H*W <= 2^34 elements
static inline bool noise_fits(int64_t frames_total, int64_t hw) {
  return frames_total > 0 && hw > 0 && hw <= ((int64_t)1 << 32) / frames_total;
}

struct PhiloxBlock { uint32_t u[4]; };

// Ten rounds of (c0,c1,c2,c3) -> (hi(M1*c2)^c1^k0, lo(M1*c2), hi(M0*c0)^c3^k1, lo(M0*c0)), the key bumped after each.
__device__ __forceinline__ PhiloxBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                     uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return PhiloxBlock{{c0, c1, c2, c3}};
}

__device__ __forceinline__ PhiloxBlock noise_block(uint64_t seed, uint32_t j, uint32_t step, uint32_t purpose) {
  return philox4x32_10(j, step, purpose, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ((a >> 9) + 0.5) * 2^-23: exact in fp32, strictly inside (0, 1)
__device__ __forceinline__ float noise_uniform(uint32_t a) { return ((float)(a >> 9) + 0.5f) * 0x1p-23f; }

// Two normals of two words: r = sqrt(-2 ln U(ua)), the angle 2*pi*U(ub); the cosine first.  Plain logf / sqrtf / sincospif,
// every product rounded on its own.
__device__ __forceinline__ void noise_normal_pair(uint32_t ua, uint32_t ub, float *zc, float *zs) {
#pragma clang fp contract(off)
  const float r = sqrtf(-2.0f * logf(noise_uniform(ua)));
  float s, k;
  sincospif(2.0f * noise_uniform(ub), &s, &k);
  *zc = r * k;
  *zs = r * s;
}

// The four normals of a block, lane by lane.
__device__ __forceinline__ void noise_normals4(const PhiloxBlock &b, float z[4]) {
  noise_normal_pair(b.u[0], b.u[1], &z[0], &z[1]);
  noise_normal_pair(b.u[2], b.u[3], &z[2], &z[3]);
}

// The normal of one element e: lane e & 3 of block e >> 2, the same value noise_normals4 puts there.
__device__ __forceinline__ float noise_normal_at(uint64_t seed, int64_t e, uint32_t step, uint32_t purpose) {
  const PhiloxBlock b = noise_block(seed, (uint32_t)(e >> 2), step, purpose);
  const int l = (int)(e & 3);
  float zc, zs;
  noise_normal_pair(l & 2 ? b.u[2] : b.u[0], l & 2 ? b.u[3] : b.u[1], &zc, &zs);
  return l & 1 ? zs : zc;
}
