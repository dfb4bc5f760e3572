// Host-side checks of the image-query entry points (csrc/imgq.hip) under AddressSanitizer + UBSan (CPU only:
// built by tests/test_imgq_host_sanitize_cpu.py with --cuda-host-only; no device code, no kernel launch): every
// invalid shape, null or aliased operand and short workspace must come back as an error code before any device
// call, and an empty batch is a no-op.  Prints "ok" and returns 0; any sanitizer report aborts the process.
#include <cstdio>

#include "../../include/dl4ss_imgq.h"

static int g_fail = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

int main() {
  // never dereferenced: every call fails its checks first or is empty.  Far enough apart that no two of the
  // (n, h, w) / (n, E) / (n, ld) extents the calls name overlap unless a check says so
  static float buf[4 << 20];
  float *img = buf, *par = buf + (1 << 20), *vec = buf + (2 << 20), *dp = buf + (3 << 20);
  int st[2] = {0, 0};
  const int P = 2418;

  CHECK(dl4ss_imgq_param_count(28, 28, 50) == P && dl4ss_imgq_param_count(24, 24, 50) == P);
  CHECK(dl4ss_imgq_param_count(26, 37, 50) == 1568 + 32 * 50 + 50 && dl4ss_imgq_dense_in(26, 37) == 32);
  CHECK(dl4ss_imgq_param_count(DL4SS_IMGQ_MAX_HW, DL4SS_IMGQ_MAX_HW, DL4SS_IMGQ_MAX_E) > 0);
  CHECK(dl4ss_imgq_param_count(23, 28, 50) == -1 && dl4ss_imgq_param_count(28, 23, 50) == -1);
  CHECK(dl4ss_imgq_param_count(DL4SS_IMGQ_MAX_HW + 1, 28, 50) == -1);
  CHECK(dl4ss_imgq_param_count(28, DL4SS_IMGQ_MAX_HW + 1, 50) == -1);
  CHECK(dl4ss_imgq_param_count(28, 28, 0) == -1 && dl4ss_imgq_param_count(28, 28, 129) == -1);
  CHECK(dl4ss_imgq_param_count(-2147483647 - 1, 2147483647, 50) == -1 && dl4ss_imgq_dense_in(0, 0) == -1);

  CHECK(dl4ss_imgq_fwd(nullptr, par, 4, 28, 28, 50, vec, nullptr) != 0);  // no images
  CHECK(dl4ss_imgq_fwd(img, nullptr, 4, 28, 28, 50, vec, nullptr) != 0);  // no parameters
  CHECK(dl4ss_imgq_fwd(img, par, 4, 28, 28, 50, nullptr, nullptr) != 0);  // no output
  CHECK(dl4ss_imgq_fwd(img, par, -1, 28, 28, 50, vec, nullptr) != 0);     // n
  CHECK(dl4ss_imgq_fwd(img, par, 1025, 28, 28, 50, vec, nullptr) != 0);   // n > 1024
  CHECK(dl4ss_imgq_fwd(img, par, 4, 23, 28, 50, vec, nullptr) != 0);      // h below the minimum
  CHECK(dl4ss_imgq_fwd(img, par, 4, 28, 49, 50, vec, nullptr) != 0);      // w above the LDS plan
  CHECK(dl4ss_imgq_fwd(img, par, 4, 28, 28, 0, vec, nullptr) != 0);       // E
  CHECK(dl4ss_imgq_fwd(img, par, 4, 28, 28, 129, vec, nullptr) != 0);     // E > 128
  CHECK(dl4ss_imgq_fwd(img, par, 4, 28, 28, 50, img, nullptr) != 0);      // in place
  CHECK(dl4ss_imgq_fwd(img, par, 4, 28, 28, 50, img + 100, nullptr) != 0);  // vec inside the images
  CHECK(dl4ss_imgq_fwd(img, par, 4, 28, 28, 50, par + 8, nullptr) != 0);    // vec inside the parameters
  CHECK(dl4ss_imgq_fwd(img, par, 0, 28, 28, 50, vec, nullptr) == 0);      // empty: no-op
  CHECK(dl4ss_imgq_fwd(img, par, 0, 23, 28, 50, vec, nullptr) != 0);      // empty, but still a bad shape

  const long long ld = 2420;
  CHECK(dl4ss_imgq_bwd(nullptr, vec, par, 4, 28, 28, 50, dp, ld, 4 * ld, nullptr) != 0);
  CHECK(dl4ss_imgq_bwd(img, nullptr, par, 4, 28, 28, 50, dp, ld, 4 * ld, nullptr) != 0);
  CHECK(dl4ss_imgq_bwd(img, vec, nullptr, 4, 28, 28, 50, dp, ld, 4 * ld, nullptr) != 0);
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 50, nullptr, ld, 4 * ld, nullptr) != 0);
  CHECK(dl4ss_imgq_bwd(img, vec, par, -3, 28, 28, 50, dp, ld, 4 * ld, nullptr) != 0);     // n
  CHECK(dl4ss_imgq_bwd(img, vec, par, 1025, 28, 28, 50, dp, ld, 1025 * ld, nullptr) != 0);
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 20, 50, dp, ld, 4 * ld, nullptr) != 0);      // w
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 64, 28, 50, dp, ld, 4 * ld, nullptr) != 0);      // h
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 200, dp, ld, 4 * ld, nullptr) != 0);     // E
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 50, dp, P - 1, 4 * ld, nullptr) != 0);   // rows shorter than P
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 50, dp, ld, 4 * ld - 1, nullptr) != 0);  // workspace too short
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 50, dp, ld, 0, nullptr) != 0);
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 50, img, ld, 4 * ld, nullptr) != 0);     // dpart aliases images
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 50, vec, ld, 4 * ld, nullptr) != 0);     // ... dvec
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 50, par, ld, 4 * ld, nullptr) != 0);     // ... params
  CHECK(dl4ss_imgq_bwd(img, vec, par, 4, 28, 28, 50, par - 100, ld, 4 * ld, nullptr) != 0);  // overlaps params
  CHECK(dl4ss_imgq_bwd(img, vec, par, 0, 28, 28, 50, dp, ld, 0, nullptr) == 0);           // empty: no-op

  CHECK(dl4ss_imgq_reduce(nullptr, 4, ld, vec, nullptr) != 0);
  CHECK(dl4ss_imgq_reduce(dp, 4, ld, nullptr, nullptr) != 0);
  CHECK(dl4ss_imgq_reduce(dp, -1, ld, vec, nullptr) != 0);
  CHECK(dl4ss_imgq_reduce(dp, 1025, ld, vec, nullptr) != 0);
  CHECK(dl4ss_imgq_reduce(dp, 4, 0, vec, nullptr) != 0);
  CHECK(dl4ss_imgq_reduce(dp, 4, ld, dp, nullptr) != 0);           // in place
  CHECK(dl4ss_imgq_reduce(dp, 4, ld, dp + 3 * ld, nullptr) != 0);  // out inside dpart
  CHECK(dl4ss_imgq_reduce(dp, 0, ld, vec, nullptr) == 0);          // empty: no-op

  CHECK(dl4ss_imgq_guard(nullptr, st, nullptr) != 0);
  CHECK(dl4ss_imgq_guard(vec, nullptr, nullptr) != 0);

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
