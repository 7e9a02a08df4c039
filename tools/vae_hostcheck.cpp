// The host half of sp_softmax_rows_long_f32 (its argument checks) under the host sanitizers: every call below must be refused
// before anything is launched, so the program needs no GPU, takes a null stream and made-up addresses that are never followed,
// and prints what each refusal said.  sp_softmax_rows_f32 is called beside it where the two must agree on a refusal.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined
//       -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined -I video-diffusion-pipeline-parallel_amd/csrc
//       -x hip tools/vae_hostcheck.cpp video-diffusion-pipeline-parallel_amd/csrc/vae.hip
//       video-diffusion-pipeline-parallel_amd/csrc/errors.hip -o vae_hostcheck
//   vae_hostcheck
//
// (the second -fsanitize is the link's; the device code is compiled without a sanitizer).  Exit status 0 when every call was
// refused with the expected text, 1 otherwise; a sanitizer report ends the program with its own status.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "../include/svdpipe.h"

static int failures = 0;

static void expect(const char *what, int rc, const char *text) {
  const char *err = sp_last_error();
  const bool ok = rc == SP_EINVAL && strstr(err, "sp_softmax_rows_long_f32") != nullptr && strstr(err, text) != nullptr;
  printf("%-40s %s  rc=%d  %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", rc, err);
  if (!ok) ++failures;
}

static const float *x = (const float *)0x10000;
static void *o = (void *)0x900000;

static int sm(const float *in, int64_t ld, void *out, int64_t ldo, int64_t rows, int cols) {
  return sp_softmax_rows_long_f32(in, ld, out, ldo, rows, cols, 0.5f, nullptr);
}

int main() {
  expect("null x", sm(nullptr, 1024, o, 1024, 4, 1024), "null pointer");
  expect("null out", sm(x, 1024, nullptr, 1024, 4, 1024), "null pointer");
  expect("cols 0", sm(x, 1024, o, 1024, 4, 0), "cols=0");
  expect("cols negative", sm(x, 1024, o, 1024, 4, -4), "cols=-4");
  expect("cols INT_MIN", sm(x, 1024, o, 1024, 4, INT_MIN), "unsupported");
  expect("cols not a multiple of 4", sm(x, 20740, o, 20740, 4, 20738), "cols=20738");
  expect("cols above 2^24", sm(x, 1 << 25, o, 1 << 25, 1, (1 << 24) + 4), "<= 16777216");
  expect("cols INT_MAX", sm(x, (int64_t)1 << 32, o, (int64_t)1 << 32, 1, INT_MAX), "unsupported");
  expect("ld < cols", sm(x, 20732, o, 20736, 4, 20736), "ld=20732");
  expect("ld not a multiple of 4", sm(x, 20738, o, 20740, 4, 20736), "ld=20738");
  expect("ld negative", sm(x, -20736, o, 20736, 4, 20736), "ld=-20736");
  expect("ldo < cols", sm(x, 20736, o, 16384, 4, 20736), "ldo=16384");
  expect("ldo not a multiple of 4", sm(x, 20736, o, 20738, 4, 20736), "ldo=20738");
  expect("rows 0", sm(x, 20736, o, 20736, 0, 20736), "rows=0");
  expect("rows negative", sm(x, 20736, o, 20736, -1, 20736), "rows=-1");
  expect("rows above one grid", sm(x, 20736, o, 20736, (int64_t)1 << 31, 20736), "rows=2147483648");
  expect("in place, ldo == ld", sm(x, 20736, (void *)x, 20736, 4, 20736), "in place needs ldo == 2 * ld");
  expect("in place, ldo == 2 * ld + 4", sm(x, 20736, (void *)x, 2 * 20736 + 4, 4, 20736), "in place needs ldo == 2 * ld");
  // the register kernel refuses the first length the streaming one exists for, in the same words
  const int rc = sp_softmax_rows_f32(x, 16388, o, 16388, 3, 16388, 0.5f, nullptr);
  const bool ok = rc == SP_EINVAL && strstr(sp_last_error(), "sp_softmax_rows_f32: rows=3 cols=16388") != nullptr;
  printf("%-40s %s  rc=%d  %s\n", "sp_softmax_rows_f32 at 16,388 columns", ok ? "refused" : "NOT REFUSED AS EXPECTED", rc,
         sp_last_error());
  if (!ok) ++failures;

  printf("%d call(s) not refused as expected\n", failures);
  return failures ? 1 : 0;
}
