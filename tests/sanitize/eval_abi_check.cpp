// Host-side checks of the target-evaluation entry points (csrc/targeteval.hip) under AddressSanitizer + UBSan (CPU
// only: built by tests/test_eval_host_sanitize_cpu.py with --cuda-host-only; no device code, no kernel launch):
// every invalid shape, index, null operand, short workspace and aliased output must come back as
// hipErrorInvalidValue (1) before any launch.  Prints "ok" and returns 0; any sanitizer report aborts the process.
#include <cstdio>

#include "../../include/dl4ss_eval.h"

static int g_fail = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

int main() {
  const int INVALID = 1;  // hipErrorInvalidValue
  // never dereferenced by the library: every call fails its checks first
  static float buf[1 << 16];
  static double ws[1 << 12], crit[64];
  float *src = buf, *est = buf + (1 << 14), *a = buf + (2 << 14), *b = buf + (3 << 14);
  int sing = 0, idx[4] = {0, 1, 0, 1}, len[8] = {0};
  const int M = 2, N = 1000;
  const long long need = dl4ss_bss_gain_ws_bytes(M, N);

  CHECK(need == 2 * (1 * 48 + 32) * 8);
  CHECK(dl4ss_bss_gain_ws_bytes(2, 4096) == need && dl4ss_bss_gain_ws_bytes(2, 4097) == 2 * (2 * 48 + 32) * 8);
  CHECK(dl4ss_bss_gain_ws_bytes(0, 10) == 0);
  CHECK(dl4ss_bss_gain_ws_bytes(-1, 10) == -1 && dl4ss_bss_gain_ws_bytes(1, 0) == -1);
  CHECK(dl4ss_bss_gain_ws_bytes(2147483647, 2147483647) > 0);  // no overflow in long long

  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 0, 1, N, ws, need, crit, &sing, nullptr) == INVALID);   // J = 0
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 5, 1, N, ws, need, crit, &sing, nullptr) == INVALID);   // J = 5
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 5, N, ws, need, crit, &sing, nullptr) == INVALID);   // Ke = 5
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 0, N, ws, need, crit, &sing, nullptr) == INVALID);   // Ke = 0
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 1, 2, N, ws, need, crit, &sing, nullptr) == INVALID);   // index 1, J 1
  int neg[1] = {-1};
  CHECK(dl4ss_bss_gain(src, est, neg, nullptr, M, 2, 1, N, ws, need, crit, &sing, nullptr) == INVALID);   // index < 0
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 2, 0, ws, need, crit, &sing, nullptr) == INVALID);   // N < 1
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 2, -5, ws, need, crit, &sing, nullptr) == INVALID);
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, -1, 2, 2, N, ws, need, crit, &sing, nullptr) == INVALID);  // M < 0
  CHECK(dl4ss_bss_gain(nullptr, est, idx, nullptr, M, 2, 2, N, ws, need, crit, &sing, nullptr) == INVALID);
  CHECK(dl4ss_bss_gain(src, nullptr, idx, nullptr, M, 2, 2, N, ws, need, crit, &sing, nullptr) == INVALID);
  CHECK(dl4ss_bss_gain(src, est, nullptr, nullptr, M, 2, 2, N, ws, need, crit, &sing, nullptr) == INVALID);
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 2, N, nullptr, need, crit, &sing, nullptr) == INVALID);
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 2, N, ws, need, nullptr, &sing, nullptr) == INVALID);
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 2, N, ws, need, crit, nullptr, nullptr) == INVALID);
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 2, N, ws, need - 1, crit, &sing, nullptr) == INVALID);  // short
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 2, N, ws, 0, crit, &sing, nullptr) == INVALID);
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, M, 2, 2, N, (char*)ws + 4, need, crit, &sing, nullptr) == INVALID);
  // only the first Ke entries of index are read (ASan would report a read behind a 2-entry array)
  int two[2] = {0, 2};
  CHECK(dl4ss_bss_gain(src, est, two, nullptr, M, 2, 2, N, ws, need, crit, &sing, nullptr) == INVALID);  // index = J
  // the grid of M * ceil(N / 4096) workgroups must fit
  CHECK(dl4ss_bss_gain(src, est, idx, nullptr, 2147483647, 2, 2, 2147483647, ws, need, crit, &sing, nullptr) ==
        INVALID);

  // dl4ss_te_assemble: (B, S, N) = (2, 3, 100) in src; outputs a, b, est
  CHECK(dl4ss_te_assemble(nullptr, len, nullptr, 2, 3, 100, 2, a, b, est, len, nullptr) == INVALID);
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 3, 100, 2, nullptr, b, est, len, nullptr) == INVALID);
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 3, 100, 2, a, nullptr, est, len, nullptr) == INVALID);
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 3, 100, 2, a, b, nullptr, len, nullptr) == INVALID);
  CHECK(dl4ss_te_assemble(src, len, nullptr, -1, 3, 100, 2, a, b, est, len, nullptr) == INVALID);  // B
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 3, 0, 2, a, b, est, len, nullptr) == INVALID);     // N < 1
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 1, 100, 2, a, b, est, len, nullptr) == INVALID);   // S < 2
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 17, 100, 2, a, b, est, len, nullptr) == INVALID);  // S > 16
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 3, 100, 1, a, b, est, len, nullptr) == INVALID);   // spk_num < 2
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 3, 100, 4, a, b, est, len, nullptr) == INVALID);   // spk_num > S
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 3, 100, 2, src + 50, b, est, len, nullptr) == INVALID);  // in place
  CHECK(dl4ss_te_assemble(src, len, nullptr, 2, 3, 100, 2, a, a + 100, est, len, nullptr) == INVALID);   // outputs overlap
  CHECK(dl4ss_te_assemble(src, len, a + 150, 2, 3, 100, 2, a, b, est, len, nullptr) == INVALID);  // output over bgd
  CHECK(dl4ss_te_assemble(src, len, nullptr, 0, 3, 100, 2, a, b, est, len, nullptr) == 0);        // empty: no-op
  CHECK(dl4ss_te_assemble(src, len, nullptr, 0, 3, 100, 5, a, b, est, len, nullptr) == INVALID);  // empty, bad shape

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
