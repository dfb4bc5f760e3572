// Host-side checks of the voiceprint entry points (csrc/voiceprint.hip) under AddressSanitizer + UBSan (CPU
// only: built by tests/test_voiceprint_host_sanitize_cpu.py with --cuda-host-only; no device code, no kernel
// launch): every invalid shape / null or aliased operand must come back as an error code before any device call,
// and an empty batch is a no-op.  Prints "ok" and returns 0; any sanitizer report aborts the process.
#include <cstdio>

#include "../../include/dl4ss_hip.h"

static int g_fail = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

int main() {
  float f[4] = {0.f, 0.f, 0.f, 0.f};
  float *a = f, *b = f + 1, *c = f + 2, *d = f + 3;  // never dereferenced: every call fails its checks first
  int iv[2] = {0, 0};
  int *i0 = iv, *i1 = iv + 1;
  const float nan = __builtin_nanf("");

  CHECK(dl4ss_vp_compact(nullptr, 5, 9, 23, 0, 0.f, nullptr, b, i0, i1, nullptr) != 0);  // no input
  CHECK(dl4ss_vp_compact(a, 5, 9, 23, 0, 0.f, nullptr, a, i0, i1, nullptr) != 0);        // in place
  CHECK(dl4ss_vp_compact(a, 5, 0, 23, 0, 0.f, nullptr, b, i0, i1, nullptr) != 0);        // T
  CHECK(dl4ss_vp_compact(a, 5, 2049, 23, 0, 0.f, nullptr, b, i0, i1, nullptr) != 0);     // T > 2048
  CHECK(dl4ss_vp_compact(a, 5, 9, 0, 0, 0.f, nullptr, b, i0, i1, nullptr) != 0);         // F
  CHECK(dl4ss_vp_compact(a, 5, 9, 23, 2, 0.f, nullptr, b, i0, i1, nullptr) != 0);        // rule
  CHECK(dl4ss_vp_compact(a, 5, 9, 23, 1, nan, nullptr, b, i0, i1, nullptr) != 0);        // NaN threshold
  CHECK(dl4ss_vp_compact(a, -1, 9, 23, 0, 0.f, nullptr, b, i0, i1, nullptr) != 0);       // n
  CHECK(dl4ss_vp_compact(a, 0, 9, 23, 0, 0.f, nullptr, b, i0, i1, nullptr) == 0);        // empty: no-op

  CHECK(dl4ss_vp_shift(a, a, 5, 9, 14, 7, 14, i0, 1, 2, nullptr) != 0);        // in place
  CHECK(dl4ss_vp_shift(a, b, 5, 9, 14, 7, 15, i0, 1, 2, nullptr) != 0);        // columns past ld
  CHECK(dl4ss_vp_shift(a, b, 5, 9, 14, 8, 7, i0, 1, 2, nullptr) != 0);         // c0 > c1
  CHECK(dl4ss_vp_shift(a, b, 5, 9, 14, -1, 7, i0, 1, 2, nullptr) != 0);        // c0 < 0
  CHECK(dl4ss_vp_shift(a, b, 5, 9, 14, 7, 14, i0, 0, 2, nullptr) != 0);        // dir
  CHECK(dl4ss_vp_shift(a, b, 5, 9, 14, 7, 14, i0, 1, 3, nullptr) != 0);        // other
  CHECK(dl4ss_vp_shift(a, b, 5, 9, 14, 7, 14, nullptr, 1, 2, nullptr) != 0);   // no lengths
  CHECK(dl4ss_vp_shift(a, b, 0, 9, 14, 7, 14, i0, 1, 2, nullptr) == 0);        // empty

  CHECK(dl4ss_vp_mean_fwd(a, 5, 9, 0, i0, b, nullptr) != 0);        // H
  CHECK(dl4ss_vp_mean_fwd(a, 5, 0, 25, i0, b, nullptr) != 0);       // T
  CHECK(dl4ss_vp_mean_fwd(a, 5, 9, 25, nullptr, b, nullptr) != 0);  // no lengths
  CHECK(dl4ss_vp_mean_fwd(a, 0, 9, 25, i0, b, nullptr) == 0);
  CHECK(dl4ss_vp_mean_bwd(a, 5, 9, 25, i0, nullptr, nullptr) != 0);  // no output
  CHECK(dl4ss_vp_mean_bwd(a, 5, 9, -3, i0, b, nullptr) != 0);
  CHECK(dl4ss_vp_mean_bwd(a, 0, 9, 25, i0, b, nullptr) == 0);

  CHECK(dl4ss_vp_colsum_parts(0) == -1 && dl4ss_vp_colsum_parts(-5) == -1);
  CHECK(dl4ss_vp_colsum_parts(1) == 1 && dl4ss_vp_colsum_parts(64) == 1 && dl4ss_vp_colsum_parts(65) == 2);
  CHECK(dl4ss_vp_colsum_parts(16064) == 251 && dl4ss_vp_colsum_parts(65535LL * 64 + 1) == -1);
  CHECK(dl4ss_vp_colsum(a, 0, 200, b, c, nullptr) != 0);                 // no rows
  CHECK(dl4ss_vp_colsum(a, 65535LL * 64 + 1, 200, b, c, nullptr) != 0);  // more blocks than a grid takes
  CHECK(dl4ss_vp_colsum(a, 45, 0, b, c, nullptr) != 0);                  // C
  CHECK(dl4ss_vp_colsum(a, 45, 200, nullptr, c, nullptr) != 0);          // no partials
  CHECK(dl4ss_vp_colsum(a, 45, 200, b, b, nullptr) != 0);                // out aliases part
  CHECK(dl4ss_vp_colsum(a, 45, 200, b, a, nullptr) != 0);                // in place

  CHECK(dl4ss_spk_memory_fwd(a, i0, b, 1025, 50, 7, c, d, nullptr) != 0);   // n > 1024
  CHECK(dl4ss_spk_memory_fwd(a, i0, b, 6, 129, 7, c, d, nullptr) != 0);     // E > 128
  CHECK(dl4ss_spk_memory_fwd(a, i0, b, 6, 50, 0, c, d, nullptr) != 0);      // M
  CHECK(dl4ss_spk_memory_fwd(a, i0, b, 6, 50, 7, a, d, nullptr) != 0);      // u aliases v
  CHECK(dl4ss_spk_memory_fwd(a, i0, b, 6, 50, 7, c, c, nullptr) != 0);      // q aliases u
  CHECK(dl4ss_spk_memory_fwd(a, nullptr, b, 6, 50, 7, c, d, nullptr) != 0); // no ids
  CHECK(dl4ss_spk_memory_fwd(a, i0, b, 0, 50, 7, c, d, nullptr) == 0);
  CHECK(dl4ss_spk_memory_bwd(a, b, c, i0, d, 6, 50, 7, a, nullptr) != 0);   // dv aliases dq
  CHECK(dl4ss_spk_memory_bwd(a, b, c, i0, d, 6, 0, 7, f, nullptr) != 0);    // E
  CHECK(dl4ss_spk_memory_bwd(a, b, c, i0, nullptr, 6, 50, 7, d, nullptr) != 0);
  CHECK(dl4ss_spk_memory_store(a, i0, 6, 50, 7, a, nullptr, nullptr) != 0);  // q aliases mem
  CHECK(dl4ss_spk_memory_store(a, i0, 2000, 50, 7, b, nullptr, nullptr) != 0);
  CHECK(dl4ss_spk_memory_store(a, i0, 0, 50, 7, b, i1, nullptr) == 0);

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
