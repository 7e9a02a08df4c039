// The host half of sp_freeu_f16 (its argument checks) and sp_freeu_ws_bytes under the host sanitizers: every call below must
// be refused before anything is launched, so the program needs no GPU, takes a null stream and made-up addresses that are
// never followed, and prints what each refusal said; the workspace size is asked for at extreme counts.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined
//       -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined -I video-diffusion-pipeline-parallel_amd/csrc
//       -x hip tools/freeu_hostcheck.cpp video-diffusion-pipeline-parallel_amd/csrc/freeu.hip
//       video-diffusion-pipeline-parallel_amd/csrc/errors.hip -o freeu_hostcheck
//   freeu_hostcheck
//
// (the second -fsanitize is the link's; the device code is compiled without a sanitizer).  Exit status 0 when every call was
// refused with the expected text and every size is what the layout says, 1 otherwise; a sanitizer report ends the program
// with its own status.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../include/svdpipe.h"

static int failures = 0;

static void expect(const char *what, int rc, const char *text) {
  const char *err = sp_last_error();
  const bool ok = rc == SP_EINVAL && strstr(err, "sp_freeu_f16") != nullptr && strstr(err, text) != nullptr;
  printf("%-36s %s  rc=%d  %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", rc, err);
  if (!ok) ++failures;
}

static void expect_size(const char *what, size_t got, size_t want) {
  printf("%-36s %zu bytes%s\n", what, got, got == want ? "" : "  UNEXPECTED");
  if (got != want) ++failures;
}

struct Call { void *cat = (void *)0x100000; int64_t ld = 2560; int n = 28, h = 9, w = 16, cl = 1280, cr = 1280; float b = 1.3f, s = 0.9f;
              int version = 2; void *ws = (void *)0x9000000; size_t ws_bytes = (size_t)1 << 40; };
static int freeu(const Call &a) {
  return sp_freeu_f16(a.cat, a.ld, a.n, a.h, a.w, a.cl, a.cr, a.b, a.s, a.version, a.ws, a.ws_bytes, nullptr);
}

int main() {
  { Call a; a.cat = nullptr; expect("null cat", freeu(a), "null pointer"); }
  { Call a; a.ws = nullptr; expect("null ws", freeu(a), "null pointer"); }
  { Call a; a.n = 0; expect("no image", freeu(a), "must be positive"); }
  { Call a; a.h = -9; expect("h negative", freeu(a), "must be positive"); }
  { Call a; a.w = INT_MIN; expect("w INT_MIN", freeu(a), "must be positive"); }
  { Call a; a.cl = 0; expect("c_left 0", freeu(a), "must be positive"); }
  { Call a; a.cr = -8; expect("c_right negative", freeu(a), "must be positive"); }
  { Call a; a.h = 1; expect("h 1", freeu(a), "at least 2"); }
  { Call a; a.w = 1; expect("w 1", freeu(a), "at least 2"); }
  { Call a; a.cl = 1288; a.ld = 2576; expect("c_left 1288", freeu(a), "multiple of 16"); }
  { Call a; a.cr = 1276; expect("c_right 1276", freeu(a), "multiple of 16"); }
  { Call a; a.ld = 2552; expect("ld below c_left + c_right", freeu(a), "at least c_left + c_right"); }
  { Call a; a.ld = -2560; expect("ld negative", freeu(a), "at least c_left + c_right"); }
  { Call a; a.ld = 2564; expect("ld no multiple of 8", freeu(a), "multiple of 8"); }
  { Call a; a.cl = a.cr = INT_MAX - 15; a.ld = INT_MAX; expect("c_left + c_right beyond int", freeu(a), "at least c_left + c_right"); }
  { Call a; a.cat = (char *)a.cat + 8; expect("cat misaligned", freeu(a), "aligned"); }
  { Call a; a.ws = (char *)a.ws + 2; expect("ws misaligned", freeu(a), "aligned"); }
  { Call a; a.version = 0; expect("version 0", freeu(a), "version 0"); }
  { Call a; a.version = 3; expect("version 3", freeu(a), "version 3"); }
  { Call a; a.b = 0.f; expect("b 0", freeu(a), "positive and finite"); }
  { Call a; a.b = -1.3f; expect("b negative", freeu(a), "positive and finite"); }
  { Call a; a.b = INFINITY; expect("b infinite", freeu(a), "positive and finite"); }
  { Call a; a.s = NAN; expect("s NaN", freeu(a), "positive and finite"); }
  { Call a; a.s = -INFINITY; expect("s -infinite", freeu(a), "positive and finite"); }
  { Call a; a.h = 4000; a.w = 128; expect("h + w above 4096", freeu(a), "too large"); }
  { Call a; a.n = INT_MAX; a.h = a.w = 2048; expect("2^31 rows and more", freeu(a), "too large"); }
  { Call a; a.n = INT_MAX / 4 - 32; a.h = a.w = 2; a.cl = 16; a.cr = 1 << 20; a.ld = (1 << 20) + 16;
    expect("more workgroups than one grid", freeu(a), "too large"); }
  { Call a; a.ws_bytes = sp_freeu_ws_bytes(a.n, a.h, a.w, a.cl, a.cr) - 1; expect("ws one byte short", freeu(a), "is below"); }
  { Call a; a.ws_bytes = 0; expect("ws_bytes 0", freeu(a), "is below"); }

  // [n*h*w] means + [n][ceil(h*w/32)][2] (min, max) + [n][ceil(c_right/64)][chunks][7][64] partials, all fp32
  expect_size("28 x 9 x 16, 1280 + 1280", sp_freeu_ws_bytes(28, 9, 16, 1280, 1280), 4u * 28 * 144 + 8u * 28 * 5 + 1792u * 28 * 20 * 1);
  expect_size("28 x 72 x 128, 640 + 320", sp_freeu_ws_bytes(28, 72, 128, 640, 320), 4u * 28 * 9216 + 8u * 28 * 288 + 1792u * 28 * 5 * 8);
  expect_size("1 x 2 x 2, 16 + 8", sp_freeu_ws_bytes(1, 2, 2, 16, 8), 4u * 4 + 8u + 1792u);
  expect_size("no image", sp_freeu_ws_bytes(0, 9, 16, 1280, 1280), 0);
  expect_size("h 1", sp_freeu_ws_bytes(1, 1, 16, 1280, 1280), 0);
  expect_size("c_left 8", sp_freeu_ws_bytes(1, 9, 16, 8, 8), 0);
  expect_size("INT_MIN everywhere", sp_freeu_ws_bytes(INT_MIN, INT_MIN, INT_MIN, INT_MIN, INT_MIN), 0);
  expect_size("INT_MAX everywhere", sp_freeu_ws_bytes(INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX), 0);
  expect_size("INT_MAX images of 2048 x 2048", sp_freeu_ws_bytes(INT_MAX, 2048, 2048, 16, 8), 0);
  expect_size("2^31 - 65 rows", sp_freeu_ws_bytes((INT_MAX - 64) / 4, 2, 2, 16, 8) > 0, 1);
  expect_size("2^30 + 2^30 channels", sp_freeu_ws_bytes(1, 2, 2, 1 << 30, 1 << 30) > 0, 1);
  expect_size("channel counts near INT_MAX", sp_freeu_ws_bytes(1, 2, 2, INT_MAX - 15, INT_MAX - 7), 0);

  printf("%d check(s) failed\n", failures);
  return failures ? 1 : 0;
}
