// Host-side checks of the optimizer entry points of include/dl4ss_optim.h under AddressSanitizer + UBSan (CPU
// only: built by tests/test_nadam_host_sanitize_cpu.py from csrc/optim.hip with --cuda-host-only and the
// sanitizers on the host side; no device code, no kernel launch).  Every call here carries an argument the
// launchers must refuse: each comes back as hipErrorInvalidValue (1) before any device call -- the shadow-segment
// arrays are walked (and their bounds checked against n) on the host, under the sanitizer, first.
// Prints "ok" and returns 0; any sanitizer report aborts the process (halt_on_error).
#include <cstdio>
#include <initializer_list>

#include "../../include/dl4ss_optim.h"

static int g_fail = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

struct Args {  // a call that would be valid (host stand-ins for the device buffers: nothing dereferences them)
  float buf[4][16];
  double part[8];
  float gnorm[2];
  int status[2], nonfinite[1];
  long long n = 16;
  int step = 7;
  double mu = 0.45, mu_next = 0.45, mu_prod = 0.004;
  const double* partp = part;
  int n_part = 8, clip_rule = DL4SS_CLIP_KERAS;
  float max_norm = 1.f;
  int* statusp = status;
  int* nonfinitep = nonfinite;
  int sticky = 0;
  int nseg = 0;
  long long seg_off[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, seg_ldy[9] = {8, 8, 8, 8, 8, 8, 8, 8, 8};
  int seg_rows[9] = {2, 2, 2, 2, 2, 2, 2, 2, 2}, seg_cols[9] = {8, 8, 8, 8, 8, 8, 8, 8, 8};
  alignas(8) unsigned short shadow[16];
  void* seg_y[9] = {shadow, shadow, shadow, shadow, shadow, shadow, shadow, shadow, shadow};

  int nadam() {
    return dl4ss_nadam(buf[0], buf[1], buf[2], buf[3], n, 2e-3f, 0.9f, 0.999f, 1e-8f, step, mu, mu_next, mu_prod,
                       statusp, nullptr, 1.f, nullptr, nseg, seg_off, seg_rows, seg_cols, seg_y, seg_ldy, partp,
                       n_part, clip_rule, max_norm, gnorm, nonfinitep, sticky, nullptr);
  }
  int adam_ex() {
    return dl4ss_adam_clipped_ex(buf[0], buf[1], buf[2], buf[3], n, 2e-4f, 0.9f, 0.999f, 1e-8f, step, statusp,
                                 nullptr, 1.f, nullptr, nseg, seg_off, seg_rows, seg_cols, seg_y, seg_ldy, partp,
                                 n_part, clip_rule, max_norm, gnorm, nonfinitep, sticky, nullptr);
  }
};

template <class F>
static void both_refuse(F&& spoil) {
  Args a;
  spoil(a);
  CHECK(a.nadam() == 1);
  Args b;
  spoil(b);
  CHECK(b.adam_ex() == 1);
}

int main() {
  both_refuse([](Args& a) { a.step = 0; });
  both_refuse([](Args& a) { a.n = -1; });
  both_refuse([](Args& a) { a.n_part = 0; });
  both_refuse([](Args& a) { a.n_part = DL4SS_CLIP_MAX_PARTS + 1; });
  both_refuse([](Args& a) { a.partp = reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.part) + 4); });
  both_refuse([](Args& a) { a.clip_rule = 2; });
  both_refuse([](Args& a) { a.clip_rule = -1; });
  both_refuse([](Args& a) { a.max_norm = 0.f; });
  both_refuse([](Args& a) { a.max_norm = -1.f; });
  both_refuse([](Args& a) { a.max_norm = __builtin_nanf(""); });
  both_refuse([](Args& a) { a.nonfinitep = nullptr; });
  both_refuse([](Args& a) { a.sticky = 1; a.statusp = nullptr; });
  // the shadow segments: too many, one past the end of the flat buffer, a row stride below the columns, a
  // misaligned destination
  both_refuse([](Args& a) { a.nseg = 9; });
  both_refuse([](Args& a) { a.nseg = -1; });
  both_refuse([](Args& a) { a.nseg = 8; a.seg_off[7] = 1; });
  both_refuse([](Args& a) { a.nseg = 1; a.seg_ldy[0] = 7; });
  both_refuse([](Args& a) { a.nseg = 1; a.seg_y[0] = a.shadow + 1; });
  both_refuse([](Args& a) { a.nseg = 1; a.seg_y[0] = nullptr; });
  for (double bad : {0.0, 1.0, -0.1, 1.5, (double)__builtin_nanf("")}) {  // the schedule: Nadam's alone
    Args a;
    a.mu = bad;
    CHECK(a.nadam() == 1);
    Args b;
    b.mu_next = bad;
    CHECK(b.nadam() == 1);
    if (bad == 0.0) continue;  // mu_prod = 0 is the product's underflow after ~900 updates: valid, below
    Args c;
    c.mu_prod = bad;
    CHECK(c.nadam() == 1);
  }
  Args e;  // n = 0: nothing to do, and nothing launched
  e.n = 0;
  CHECK(e.nadam() == 0 && e.adam_ex() == 0);
  e.mu_prod = 0.0;  // accepted (n = 0: the arguments are checked, nothing is launched)
  CHECK(e.nadam() == 0);
  e.mu_prod = 4.9406564584124654e-324;  // and the smallest denormal, where the default schedule's product sticks
  CHECK(e.nadam() == 0);
  if (g_fail) return 1;
  std::puts("ok");
  return 0;
}
