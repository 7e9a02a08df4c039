// The host half of sp_attn_temporal_long_f16 (its argument checks) under the host sanitizers, as tools/attn_kv_hostcheck.cpp
// (the command line is in README.md): every call is refused before anything is launched -- no GPU, a null stream, made-up
// addresses that are never followed.  Exit status 0 when every call was refused with the expected text, else 1.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../include/svdpipe.h"

struct Attn { const void *q = (const void *)0x10000, *k = (const void *)0x20000, *v = (const void *)0x30000;
              const void *o = (const void *)0xb00000; int64_t ldq = 960, ldk = 960, ldv = 960, ldo = 320; int batch = 1, frames = 48;
              int64_t hw = 9216; int heads = 5; float scale = 0.125f; const void *zero = (const void *)0xc00000; };
static int failures = 0;

template <class F> static void refused(const char *what, const char *text, F change) {
  Attn a;
  change(a);
  const int rc = sp_attn_temporal_long_f16(a.q, a.k, a.v, (void *)a.o, a.ldq, a.ldk, a.ldv, a.ldo, a.batch, a.frames, a.hw, a.heads,
                                           a.scale, a.zero, nullptr);
  const char *err = sp_last_error();
  const bool ok = rc == SP_EINVAL && strstr(err, "sp_attn_temporal_long_f16") && strstr(err, text);
  printf("%-28s %s  rc=%d  %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", rc, err);
  failures += !ok;
}

int main() {
  for (auto m : {&Attn::q, &Attn::k, &Attn::v, &Attn::o, &Attn::zero}) refused("null pointer", "null pointer", [m](Attn &a) { a.*m = nullptr; });
  for (int f : {INT_MIN, -48, 0, 1, 25, 32, 129, 256, INT_MAX}) refused("frames out of range", "[33,128]", [f](Attn &a) { a.frames = f; });
  for (int n : {0, -1, INT_MIN}) refused("batch not positive", "must be positive", [n](Attn &a) { a.batch = n; });
  for (int64_t n : {(int64_t)0, INT64_MIN}) refused("hw not positive", "must be positive", [n](Attn &a) { a.hw = n; });
  refused("heads negative", "must be positive", [](Attn &a) { a.heads = -5; });
  for (auto m : {&Attn::ldq, &Attn::ldk, &Attn::ldv, &Attn::ldo})
    for (int64_t ld : {(int64_t)312, (int64_t)0, (int64_t)-960}) refused("pitch below heads*64", "at least heads*64", [m, ld](Attn &a) { a.*m = ld; });
  refused("heads INT_MAX", "at least heads*64", [](Attn &a) { a.heads = INT_MAX; });
  for (auto m : {&Attn::ldq, &Attn::ldk, &Attn::ldv, &Attn::ldo}) refused("pitch no multiple of 8", "multiples of 8", [m](Attn &a) { a.*m = 964; });
  for (auto m : {&Attn::q, &Attn::k, &Attn::v, &Attn::o, &Attn::zero})
    for (int off : {2, 8}) refused("misaligned pointer", "16-byte aligned", [m, off](Attn &a) { a.*m = (const char *)(a.*m) + off; });
  for (float s : {0.f, -0.125f, INFINITY, NAN}) refused("scale not positive and finite", "positive and finite", [s](Attn &a) { a.scale = s; });
  refused("more problems than a grid", "too large", [](Attn &a) { a.batch = INT_MAX; a.hw = INT64_MAX; });
  refused("2^40 pixels", "too large", [](Attn &a) { a.batch = 1 << 20; a.hw = 1 << 20; });
  printf("%d call(s) not refused as expected\n", failures);
  return failures ? 1 : 0;
}
