// Host-side checks of the device-resident corpus entry points (csrc/corpus/corpus.hip) under AddressSanitizer +
// UBSan (CPU only: built by tests/test_corpus_host_sanitize_cpu.py with --cuda-host-only; no device code, no kernel
// launch): every null pointer, bad source count, misaligned pool, unknown dtype and N < 1 must come back as an
// error code before any device call, and an empty batch / corpus is a no-op.  Prints "ok" and returns 0; any
// sanitizer report aborts the process.
#include <cstdio>

#include "../../include/corpus/dl4ss_corpus.h"

static int g_fail = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

int main() {
  // never dereferenced: every call fails its checks first or is empty
  alignas(16) static float buf[1 << 16];
  static long long off[4];
  static int ints[256];
  void* pool = buf;
  float *ws = buf + 4096, *stats = buf + 8192, *gains = buf + 12288, *src = buf + 16384, *mix = buf + 32768;
  int *len = ints, *clips = ints + 64, *shifts = ints + 128, *out_len = ints + 192, *bad = ints + 250;
  const int I16 = DL4SS_CORPUS_I16, F32 = DL4SS_CORPUS_F32;

  CHECK(dl4ss_corpus_stats(nullptr, I16, off, len, 4, ws, stats, nullptr) != 0);    // no pool
  CHECK(dl4ss_corpus_stats(pool, I16, nullptr, len, 4, ws, stats, nullptr) != 0);   // no offsets
  CHECK(dl4ss_corpus_stats(pool, I16, off, nullptr, 4, ws, stats, nullptr) != 0);   // no lengths
  CHECK(dl4ss_corpus_stats(pool, I16, off, len, 4, nullptr, stats, nullptr) != 0);  // no workspace
  CHECK(dl4ss_corpus_stats(pool, I16, off, len, 4, ws, nullptr, nullptr) != 0);     // no output
  CHECK(dl4ss_corpus_stats(pool, 2, off, len, 4, ws, stats, nullptr) != 0);         // unknown dtype
  CHECK(dl4ss_corpus_stats(pool, -1, off, len, 4, ws, stats, nullptr) != 0);
  CHECK(dl4ss_corpus_stats(pool, F32, off, len, -1, ws, stats, nullptr) != 0);      // n_clips
  CHECK(dl4ss_corpus_stats(buf + 1, F32, off, len, 4, ws, stats, nullptr) != 0);    // misaligned pool
  CHECK(dl4ss_corpus_stats(pool, F32, off, len, 4, ws + 1, stats, nullptr) != 0);   // misaligned workspace
  CHECK(dl4ss_corpus_stats(pool, F32, off, len, 4, ws, stats + 1, nullptr) != 0);   // misaligned float2 output
  CHECK(dl4ss_corpus_stats(pool, F32, off, len, 0, ws, stats, nullptr) == 0);       // empty corpus: no-op
  CHECK(dl4ss_corpus_stats(pool, 7, off, len, 0, ws, stats, nullptr) != 0);         // empty, but still a bad dtype

#define MIX(pool_, dt, off_, len_, st, n, cl, sh, g, B, K, Ks, N, s, m, ol, bd) \
  dl4ss_mix_corpus(pool_, dt, off_, len_, st, n, cl, sh, g, B, K, Ks, N, s, m, ol, bd, nullptr)
  CHECK(MIX(nullptr, I16, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, nullptr, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, nullptr, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, nullptr, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, nullptr, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, nullptr, 2, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, nullptr, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, nullptr, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, nullptr) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 0, 2, 400, src, mix, out_len, bad) != 0);   // K < 1
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, -1, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 3, 2, 400, src, mix, out_len, bad) != 0);   // Ks < K
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 2, 17, 400, src, mix, out_len, bad) != 0);  // Ks > 16
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 17, 17, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 0, src, mix, out_len, bad) != 0);     // N < 1
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, -8, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, -1, 2, 2, 400, src, mix, out_len, bad) != 0);  // B
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, shifts, gains, 65536, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, I16, off, len, stats, 0, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);   // no clips
  CHECK(MIX(pool, 2, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);     // dtype
  CHECK(MIX(buf + 2, F32, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);  // pool
  CHECK(MIX((char*)pool + 8, I16, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, F32, off, len, stats + 1, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix, out_len, bad) != 0);
  CHECK(MIX(pool, F32, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src + 1, mix, out_len, bad) != 0);  // 16-B stores
  CHECK(MIX(pool, F32, off, len, stats, 4, clips, shifts, gains, 2, 2, 2, 400, src, mix + 2, out_len, bad) != 0);
  // empty batch: a no-op, with or without the optional arrays; a bad shape is still refused
  CHECK(MIX(pool, F32, off, len, stats, 4, clips, shifts, gains, 0, 2, 3, 400, src, mix, out_len, bad) == 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, nullptr, gains, 0, 1, 1, 401, src + 1, mix + 1, nullptr, bad) == 0);
  CHECK(MIX(pool, I16, off, len, stats, 4, clips, nullptr, gains, 0, 2, 1, 400, src, mix, nullptr, bad) != 0);

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
