// The host half of the tiles entry points (argument checks and plan arithmetic of sp_euler_step_tiles_f16 and
// sp_dpmpp2m_step_tiles_f16) under the host sanitizers: every call below must be refused before anything is launched, so the
// program needs no GPU, takes a null stream and made-up addresses that are never followed, and prints what each refusal said.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined
//       -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined -I video-diffusion-pipeline-parallel_amd/csrc
//       -x hip tools/tile_hostcheck.cpp video-diffusion-pipeline-parallel_amd/csrc/sampler_tail.hip
//       video-diffusion-pipeline-parallel_amd/csrc/noise.hip video-diffusion-pipeline-parallel_amd/csrc/errors.hip
//       -o tile_hostcheck
//   tile_hostcheck
//
// (the second -fsanitize is the link's; the device code is compiled without a sanitizer).  Exit status 0 when every call was
// refused with the expected text, 1 otherwise; a sanitizer report ends the program with its own status.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../include/svdpipe.h"

static int failures = 0;

static void expect(const char *what, int rc, const char *text) {
  const char *err = sp_last_error();
  const bool ok = rc == SP_EINVAL && strstr(err, text) != nullptr;
  printf("%-44s %s  rc=%d  %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", rc, err);
  if (!ok) ++failures;
}

static const void *x = (const void *)0x10000, *e = (const void *)0x20000;
static void *o = (void *)0x30000;
static const uint64_t *seeds = (const uint64_t *)0x50000, *odd = (const uint64_t *)0x50004;

// 6 frames as windows of 4, 2 apart; 6 x 12 cells as tiles of 4 x 8, 2 x 4 apart: 2 x 2 x 2 patches
static sp_tile_plan good() {
  sp_tile_plan p;
  p.frames_total = 6; p.window = 4; p.stride = 2; p.n_win = 2;
  p.h = 6; p.w = 12; p.tile_h = 4; p.tile_w = 8; p.stride_y = 2; p.stride_x = 4; p.n_ty = 2; p.n_tx = 2;
  p.wf = (const float *)0x40000; p.wy = (const float *)0x41000; p.wx = (const float *)0x42000;
  return p;
}

static int euler(const sp_tile_plan *p, const void *lat = x, void *out = o, float sigma = 2.f, float n = 0.f,
                 const uint64_t *sd = nullptr, const void *eu = nullptr, const float *g = nullptr, int64_t ld_g = 0, int batch = 1,
                 int64_t ld_eps = 4) {
  return sp_euler_step_tiles_f16(p, lat, e, eu, ld_eps, g, ld_g, out, sigma, 1.f, batch, n, sd, 0, nullptr);
}

static int solver(const sp_tile_plan *p, float a = .5f, float c2 = 0.f, float n = 0.f, const uint64_t *sd = nullptr) {
  return sp_dpmpp2m_step_tiles_f16(p, x, e, nullptr, 4, nullptr, 0, o, 2.f, a, .5f, 1.f, c2, 1, n, sd, 0, nullptr);
}

int main() {
  sp_tile_plan p = good();
  if (sp_tile_plan_size() != sizeof(sp_tile_plan)) { printf("sp_tile_plan_size() disagrees with the header\n"); ++failures; }

  expect("euler: null plan", euler(nullptr), "null plan");
  p = good(); p.wf = nullptr; expect("euler: null wf", euler(&p), "null table");
  p = good(); p.wy = nullptr; expect("euler: null wy", euler(&p), "null table");
  p = good(); p.wx = nullptr; expect("2m: null wx", solver(&p), "null table");
  p = good(); p.stride_y = 0; expect("euler: stride_y 0", euler(&p), "y (total, tile, stride) = (6, 4, 0)");
  p = good(); p.stride_x = 9; expect("euler: stride_x > tile", euler(&p), "x (total, tile, stride) = (12, 8, 9)");
  p = good(); p.stride_x = INT_MIN; expect("euler: stride_x INT_MIN", euler(&p), "stride must be from 1");
  p = good(); p.w = 13; expect("euler: w not tile + strides", euler(&p), "x (total, tile, stride) = (13, 8, 4)");
  p = good(); p.h = 7; expect("2m: h not tile + strides", solver(&p), "y (total, tile, stride) = (7, 4, 2)");
  p = good(); p.tile_h = 7; expect("euler: tile exceeds total", euler(&p), "the tile exceeds the total");
  p = good(); p.h = INT_MAX; p.tile_h = 1; p.stride_y = 1; p.n_ty = 2; expect("euler: INT_MAX rows, n_ty", euler(&p), "n_ty=2");
  p = good(); p.n_ty = 3; expect("euler: n_ty not the plan's", euler(&p), "n_ty=3");
  p = good(); p.n_tx = 1; expect("2m: n_tx not the plan's", solver(&p), "n_tx=1");
  p = good(); p.tile_w = 0; expect("euler: tile_w 0", euler(&p), "dims");
  p = good(); p.h = -6; expect("euler: negative h", euler(&p), "dims");
  p = good(); p.stride = 0; expect("euler: frame stride 0", euler(&p), "stride=0");
  p = good(); p.frames_total = 7; expect("euler: frames not window + strides", euler(&p), "whole number of strides");
  p = good(); p.n_win = 3; expect("2m: n_win not the plan's", solver(&p), "n_win");
  p = good(); p.window = 8; expect("euler: window exceeds total", euler(&p), "exceeds");
  p = good();
  expect("euler: null latent", euler(&p, nullptr), "null pointer");
  expect("euler: batch 0", euler(&p, x, o, 2.f, 0.f, nullptr, nullptr, nullptr, 0, 0), "dims");
  expect("euler: ld_eps 6", euler(&p, x, o, 2.f, 0.f, nullptr, nullptr, nullptr, 0, 1, 6), "ld_eps");
  expect("euler: sigma 0", euler(&p, x, o, 0.f), "sigma");
  expect("euler: CFG without guidance", euler(&p, x, o, 2.f, 0.f, nullptr, e), "guidance");
  expect("euler: ld_guidance in (0, window)", euler(&p, x, o, 2.f, 0.f, nullptr, e, (const float *)0x60000, 3), "ld_guidance");
  expect("euler: overlapping out", euler(&p, x, (char *)x + 2), "overlap");
  expect("euler: null seeds with noise", euler(&p, x, o, 2.f, .5f, nullptr), "null seeds");
  expect("euler: misaligned seeds", euler(&p, x, o, 2.f, .5f, odd), "8-byte aligned");
  expect("euler: negative noise_scale", euler(&p, x, o, 2.f, -.5f, seeds), "noise_scale");
  expect("euler: NaN noise_scale", euler(&p, x, o, 2.f, NAN, seeds), "noise_scale");
  expect("2m: infinite noise_scale", solver(&p, .5f, 0.f, INFINITY, seeds), "noise_scale");
  expect("2m: a = 1", solver(&p, 1.f), "a = ");
  expect("2m: negative c2", solver(&p, .5f, -1.f), "c2");
  // one tile of 65536 x 65536 cells, two frames: 4*F*H*W = 2^35
  p = good(); p.frames_total = p.window = p.stride = 2; p.n_win = 1;
  p.h = p.w = p.tile_h = p.tile_w = p.stride_y = p.stride_x = 65536; p.n_ty = p.n_tx = 1;
  expect("euler: 4*F*H*W > 2^34", euler(&p, x, (void *)x), "2^34");
  expect("2m: 4*F*H*W > 2^34, with noise", sp_dpmpp2m_step_tiles_f16(&p, x, e, nullptr, 4, nullptr, 0, (void *)x, 2.f, .5f, .5f, 1.f, 0.f, 1, .5f, seeds, 0, nullptr), "2^34");

  printf("%d call(s) not refused as expected\n", failures);
  return failures ? 1 : 0;
}
