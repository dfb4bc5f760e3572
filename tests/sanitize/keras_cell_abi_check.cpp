// Host-side checks of the recurrence entry points' DL4SS_RNN_HARD_GATES dispatch (csrc/birnn.hip) under
// AddressSanitizer + UBSan (CPU only: built by tests/test_keras_cell_host_sanitize_cpu.py with --cuda-host-only; no
// device code, no kernel launch): the flag is accepted with DL4SS_CELL_LSTM and base precision 0 only, and every
// other combination must come back as hipErrorInvalidValue (1) before any device call.  Prints "ok" and returns 0;
// any sanitizer report aborts the process.
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
  float f[8] = {0.f};
  float *G = f, *W = f + 1, *b = f + 2, *out = f + 3, *hp = f + 4, *act = f + 5, *cs = f + 6, *dG = f + 7;
  // never dereferenced: every call fails its checks first
  unsigned short h16[2] = {0, 0};
  long long ws[4] = {0, 0, 0, 0};
  int st = 0;
  const int B = 4, T = 2, H = 40, HARD = DL4SS_RNN_HARD_GATES;
  const long long wsb = 1LL << 30;
  const int INVALID = 1;  // hipErrorInvalidValue

  static_assert(DL4SS_RNN_HARD_GATES == 0x800, "the flag's value");
  static_assert((DL4SS_RNN_HARD_GATES & (DL4SS_RNN_WS_ZEROED | DL4SS_RNN_DGH_PAD8 | DL4SS_RNN_DEFER_BIAS |
                                         DL4SS_RNN_DOUT_SLABS_MASK | 0xFF)) == 0, "disjoint from the other fields");

  // ---- forward: GRU, precision 1, out_bf16, hprev_bf16, h_mean, no fp32 output
  CHECK(dl4ss_birnn_fwd(DL4SS_CELL_GRU, HARD, B, T, H, G, W, b, out, hp, act, cs, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_fwd(DL4SS_CELL_LSTM, HARD | 1, B, T, H, G, W, b, out, hp, act, cs, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_fwd(2, HARD, B, T, H, G, W, b, out, hp, act, cs, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_fwd_ex(DL4SS_CELL_LSTM, HARD, B, T, H, G, W, b, out, hp, act, cs, h16, nullptr, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_fwd_ex(DL4SS_CELL_LSTM, HARD, B, T, H, G, W, b, out, hp, act, cs, nullptr, h16, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_fwd_mean(DL4SS_CELL_LSTM, HARD, B, T, H, G, W, b, out, hp, act, cs, nullptr, nullptr, out, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_fwd_mean(DL4SS_CELL_LSTM, HARD, B, T, H, G, W, b, nullptr, hp, act, cs, h16, nullptr, nullptr, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_fwd_mean(DL4SS_CELL_LSTM, HARD | DL4SS_RNN_WS_ZEROED | 1, B, T, H, G, W, b, out, hp, act, cs, nullptr, nullptr, nullptr, ws, wsb, &st, nullptr) == INVALID);
  // an unknown bit next to the flag is still refused (the base precision must be 0)
  CHECK(dl4ss_birnn_fwd(DL4SS_CELL_LSTM, HARD | 2, B, T, H, G, W, b, out, hp, act, cs, ws, wsb, &st, nullptr) == INVALID);
  // the large-H limit holds with the flag
  CHECK(dl4ss_birnn_fwd(DL4SS_CELL_LSTM, HARD, B, T, 641, G, W, b, out, hp, act, cs, ws, wsb, &st, nullptr) != 0);

  // ---- BPTT: GRU, precision 1, bf16 dG / dGh, dOut slabs, no fp32 dG
  CHECK(dl4ss_birnn_bwd(DL4SS_CELL_GRU, HARD, B, T, H, out, nullptr, W, act, cs, hp, dG, dG, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_bwd(DL4SS_CELL_LSTM, HARD | 1, B, T, H, out, nullptr, W, act, cs, hp, dG, nullptr, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_bwd_ex(DL4SS_CELL_LSTM, HARD, B, T, H, out, nullptr, W, act, cs, hp, dG, nullptr, h16, nullptr, nullptr, nullptr, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_bwd_ex(DL4SS_CELL_LSTM, HARD, B, T, H, out, nullptr, W, act, cs, hp, dG, nullptr, nullptr, h16, nullptr, nullptr, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_bwd_ex(DL4SS_CELL_LSTM, HARD, B, T, H, out, nullptr, W, act, cs, hp, nullptr, nullptr, h16, nullptr, nullptr, nullptr, ws, wsb, &st, nullptr) == INVALID);
  for (int s = 2; s <= 4; ++s)
    CHECK(dl4ss_birnn_bwd_ex(DL4SS_CELL_LSTM, HARD | DL4SS_RNN_DOUT_SLABS(s), B, T, H, out, nullptr, W, act, cs, hp, dG, nullptr, nullptr, nullptr, nullptr, nullptr, ws, wsb, &st, nullptr) == INVALID);
  CHECK(dl4ss_birnn_bwd_ex(DL4SS_CELL_LSTM, HARD, B, T, 641, out, nullptr, W, act, cs, hp, dG, nullptr, nullptr, nullptr, nullptr, nullptr, ws, wsb, &st, nullptr) != 0);
  // the plain entry point keeps its H <= 320 limit with the flag
  CHECK(dl4ss_birnn_bwd(DL4SS_CELL_LSTM, HARD, B, T, 600, out, nullptr, W, act, cs, hp, dG, nullptr, ws, wsb, &st, nullptr) == INVALID);

  // the plan and the workspace size are the LSTM's: host-only queries, untouched by the flag's existence
  int info[5] = {0, 0, 0, 0, 0};
  CHECK(dl4ss_birnn_plan_info(DL4SS_CELL_LSTM, 5, 25, 0, 240, info) == 0 && info[0] == 1 && info[1] == 2 && info[2] == 20);
  CHECK(st == 0);
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
