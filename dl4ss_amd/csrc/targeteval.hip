// Target-speaker evaluation (include/dl4ss_eval.h): BSS Eval 2.0's gain decomposition, batched, and the
// evaluation mixture in the reference's summation order (Cocktail/software/DL4SS_Keras/predict.py:46-336,
// BSS_EVAL.m: bss_decomp_gain + bss_crit).
//
// dl4ss_bss_gain is four launches over caller-owned workspace, no atomics:
//   pass 1   workgroup (m, chunk): fp64 partial sums of G (lower triangle), d and |e|^2 over its 4096 samples
//   solve    thread (m, e): the chunks' partials added in ascending order, G = L D L^T over the sources of
//            non-zero energy, c, a, |s_target|^2 and the singular flag
//   pass 2   workgroup (m, chunk): partial sums of (e - P)^2, (P - a s)^2, (e - a s)^2, P^2 from the samples
//   final    one workgroup: chunks added in ascending order, the criteria, the singular count
// A lane owns the samples chunk * 4096 + lane + 256 k, the wave reduces by the xor butterfly (each pair forms
// the same sum on both sides: one fixed tree), then the four waves are added in ascending order.  The loads are
// one dword per lane: consecutive lanes read consecutive samples (256 B per wave and load), and rows start at
// multiples of N floats, which need not be 16-B aligned.  2 (J + Ke) N 4 B per utterance cross HBM / L2.
#include "common.h"

#include "../../include/dl4ss_eval.h"

// No contraction in this file: every fused multiply-add is written as fma().  Fused by the compiler, P - a s_idx
// would keep the product a s_idx unrounded, and an estimate that lies exactly in the span (J = 1: P = a s_idx, so
// SIR = +inf) would leave the product's rounding error behind as an interference of -320 dB.
#pragma clang fp contract(off)

namespace {

constexpr int kChunk = DL4SS_BSS_GAIN_CHUNK;
constexpr int kThreads = 256;
constexpr int kP1 = 32;   // doubles per (m, chunk) of pass 1: 10 + 16 + 4 used at J = Ke = 4
constexpr int kP2 = 16;   // doubles per (m, chunk) of pass 2: 4 per estimate
constexpr int kCoef = 8;  // doubles per (m, e): c[0..3], a, flag, |s_target|^2, unused

struct GainIndex {
  int v[DL4SS_BSS_GAIN_MAX_SRC];
};

__host__ __device__ inline long long gain_nchunk(int N) { return ((long long)N + kChunk - 1) / kChunk; }

__device__ __forceinline__ int eff_len(const int* n_eff, int m, int N) {
  if (!n_eff) return N;
  const int n = n_eff[m];
  return n < 0 ? 0 : (n > N ? N : n);
}

// the block's sums of acc[0..NP): waves in ascending order, written by the first NP threads
template <int NP>
__device__ __forceinline__ void block_sums(double (&acc)[NP], double* out) {
  __shared__ double sh[kThreads / 64][NP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const double v = wave_sum_d(acc[i]);
    if (lane == 0) sh[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < NP) {
    double s = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += sh[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

template <int J, int KE>
__global__ __launch_bounds__(kThreads) void gain_pass1_kernel(const float* __restrict__ src,
                                                              const float* __restrict__ est,
                                                              const int* __restrict__ n_eff, int N, int nchunk,
                                                              double* __restrict__ p1) {
  constexpr int NG = J * (J + 1) / 2, NP = NG + J * KE + KE;
  const long long blk = blockIdx.x;
  const int m = (int)(blk / nchunk), c = (int)(blk % nchunk);
  const int n = eff_len(n_eff, m, N);
  const long long lo = (long long)c * kChunk;
  const long long hi = lo + kChunk < n ? lo + kChunk : n;
  const float* s0 = src + (long long)m * J * N;
  const float* e0 = est + (long long)m * KE * N;
  double acc[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) acc[i] = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += kThreads) {
    double s[J], e[KE];
#pragma unroll
    for (int j = 0; j < J; ++j) s[j] = (double)s0[(long long)j * N + i];
#pragma unroll
    for (int k = 0; k < KE; ++k) e[k] = (double)e0[(long long)k * N + i];
    int p = 0;
#pragma unroll
    for (int a = 0; a < J; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        acc[p] = fma(s[a], s[b], acc[p]);
        ++p;
      }
#pragma unroll
    for (int k = 0; k < KE; ++k)
#pragma unroll
      for (int j = 0; j < J; ++j) {
        acc[p] = fma(e[k], s[j], acc[p]);
        ++p;
      }
#pragma unroll
    for (int k = 0; k < KE; ++k) {
      acc[p] = fma(e[k], e[k], acc[p]);
      ++p;
    }
  }
  block_sums<NP>(acc, p1 + blk * kP1);
}

template <int J, int KE>
__global__ void gain_solve_kernel(const double* __restrict__ p1, int M, int nchunk, GainIndex index,
                                  double* __restrict__ coef) {
  constexpr int NG = J * (J + 1) / 2;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)M * KE) return;
  const int m = (int)(t / KE), e = (int)(t % KE);
  double g[NG], d[J];
#pragma unroll
  for (int i = 0; i < NG; ++i) g[i] = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j) d[j] = 0.0;
  for (int c = 0; c < nchunk; ++c) {  // ascending chunk order
    const double* p = p1 + ((long long)m * nchunk + c) * kP1;
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] += p[i];
#pragma unroll
    for (int j = 0; j < J; ++j) d[j] += p[NG + e * J + j];
  }
  double G[J][J];
  {
    int p = 0;
#pragma unroll
    for (int a = 0; a < J; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        G[a][b] = g[p];
        G[b][a] = g[p];
        ++p;
      }
  }
  bool act[J];
#pragma unroll
  for (int j = 0; j < J; ++j) act[j] = G[j][j] > 0.0;  // a silent source is left out of the span
  // G = L D L^T over the active sources, ascending; D_j is the Cholesky pivot (before its square root)
  double L[J][J], D[J];
  bool singular = false;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    D[j] = 1.0;
#pragma unroll
    for (int k = 0; k < J; ++k) L[j][k] = 0.0;
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (!act[j]) continue;
    double piv = G[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k)
      if (act[k]) piv -= L[j][k] * L[j][k] * D[k];
    if (!(piv > 1e-12 * G[j][j])) singular = true;
    D[j] = piv;
#pragma unroll
    for (int i = j + 1; i < J; ++i) {
      if (!act[i]) continue;
      double v = G[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k)
        if (act[k]) v -= L[i][k] * L[j][k] * D[k];
      L[i][j] = v / piv;
    }
  }
  double z[J], c[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {  // L z = d
    double v = act[j] ? d[j] : 0.0;
#pragma unroll
    for (int k = 0; k < j; ++k)
      if (act[k]) v -= L[j][k] * z[k];
    z[j] = v;
  }
#pragma unroll
  for (int j = J - 1; j >= 0; --j) {  // L^T c = D^{-1} z
    double v = act[j] ? z[j] / D[j] : 0.0;
#pragma unroll
    for (int k = j + 1; k < J; ++k)
      if (act[k]) v -= L[k][j] * c[k];
    c[j] = act[j] ? v : 0.0;
  }
  double gii = 0.0, di = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j)  // (a select, not a dynamic index: the arrays stay in registers)
    if (j == index.v[e]) {
      gii = G[j][j];
      di = d[j];
    }
  const double a = di / gii;
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  double* o = coef + t * kCoef;
#pragma unroll
  for (int j = 0; j < DL4SS_BSS_GAIN_MAX_SRC; ++j) o[j] = j < J ? (singular ? nan : c[j]) : 0.0;
  o[4] = singular ? nan : a;
  o[5] = singular ? 1.0 : 0.0;
  o[6] = singular ? nan : a * a * gii;
  o[7] = 0.0;
}

template <int J, int KE>
__global__ __launch_bounds__(kThreads) void gain_pass2_kernel(const float* __restrict__ src,
                                                              const float* __restrict__ est,
                                                              const int* __restrict__ n_eff, int N, int nchunk,
                                                              GainIndex index, const double* __restrict__ coef,
                                                              double* __restrict__ p2) {
  const long long blk = blockIdx.x;
  const int m = (int)(blk / nchunk), c = (int)(blk % nchunk);
  const int n = eff_len(n_eff, m, N);
  const long long lo = (long long)c * kChunk;
  const long long hi = lo + kChunk < n ? lo + kChunk : n;
  const float* s0 = src + (long long)m * J * N;
  const float* e0 = est + (long long)m * KE * N;
  double cf[KE][J], a[KE];
#pragma unroll
  for (int k = 0; k < KE; ++k) {
    const double* o = coef + ((long long)m * KE + k) * kCoef;
#pragma unroll
    for (int j = 0; j < J; ++j) cf[k][j] = o[j];
    a[k] = o[4];
  }
  double acc[4 * KE];
#pragma unroll
  for (int i = 0; i < 4 * KE; ++i) acc[i] = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += kThreads) {
    double s[J];
#pragma unroll
    for (int j = 0; j < J; ++j) s[j] = (double)s0[(long long)j * N + i];
#pragma unroll
    for (int k = 0; k < KE; ++k) {
      const double e = (double)e0[(long long)k * N + i];
      double P = 0.0, si = 0.0;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        P = fma(cf[k][j], s[j], P);
        if (j == index.v[k]) si = s[j];
      }
      const double t = a[k] * si;
      const double r0 = e - P, r1 = P - t, r2 = e - t;
      acc[4 * k + 0] = fma(r0, r0, acc[4 * k + 0]);
      acc[4 * k + 1] = fma(r1, r1, acc[4 * k + 1]);
      acc[4 * k + 2] = fma(r2, r2, acc[4 * k + 2]);
      acc[4 * k + 3] = fma(P, P, acc[4 * k + 3]);
    }
  }
  block_sums<4 * KE>(acc, p2 + blk * kP2);
}

__device__ __forceinline__ double crit_db(double num, double den) { return 10.0 * log10(num / den); }

__global__ __launch_bounds__(kThreads) void gain_final_kernel(const double* __restrict__ coef,
                                                              const double* __restrict__ p2, int M, int KE,
                                                              int nchunk, double* __restrict__ crit,
                                                              int* __restrict__ singular) {
  __shared__ int cnt[kThreads];
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  int mine = 0;
  const long long pairs = (long long)M * KE;
  for (long long t = threadIdx.x; t < pairs; t += kThreads) {
    const long long m = t / KE;
    const int e = (int)(t % KE);
    double en[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunk; ++c) {  // ascending chunk order
      const double* p = p2 + (m * nchunk + c) * kP2 + 4 * e;
#pragma unroll
      for (int i = 0; i < 4; ++i) en[i] += p[i];
    }
    const double* o = coef + t * kCoef;
    double* out = crit + t * 3;
    if (o[5] != 0.0) {
      ++mine;
      out[0] = out[1] = out[2] = nan;
    } else {
      const double st = o[6];
      out[0] = crit_db(st, en[2]);     // |s_target|^2 / |e_interf + e_artif|^2
      out[1] = crit_db(st, en[1]);     // |s_target|^2 / |e_interf|^2
      out[2] = crit_db(en[3], en[0]);  // |s_target + e_interf|^2 / |e_artif|^2
    }
  }
  cnt[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < kThreads; ++i) s += cnt[i];
    singular[0] = s;
  }
}

template <int J, int KE>
int gain_launch(const float* src, const float* est, const GainIndex& index, const int* n_eff, int M, int N, double* ws,
                double* crit, int* singular, hipStream_t st) {
  const int nchunk = (int)gain_nchunk(N);
  double* p1 = ws;
  double* coef = p1 + (long long)M * nchunk * kP1;
  double* p2 = coef + (long long)M * DL4SS_BSS_GAIN_MAX_SRC * kCoef;
  const unsigned grid = (unsigned)((long long)M * nchunk);
  hipLaunchKernelGGL((gain_pass1_kernel<J, KE>), dim3(grid), dim3(kThreads), 0, st, src, est, n_eff, N, nchunk, p1);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL((gain_solve_kernel<J, KE>), dim3(cdiv((long long)M * KE, 64)), dim3(64), 0, st, p1, M, nchunk,
                     index, coef);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL((gain_pass2_kernel<J, KE>), dim3(grid), dim3(kThreads), 0, st, src, est, n_eff, N, nchunk, index,
                     coef, p2);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL(gain_final_kernel, dim3(1), dim3(kThreads), 0, st, coef, p2, M, KE, nchunk, crit, singular);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

template <int J>
int gain_launch_j(int Ke, const float* src, const float* est, const GainIndex& index, const int* n_eff, int M, int N,
                  double* ws, double* crit, int* singular, hipStream_t st) {
  switch (Ke) {
    case 1: return gain_launch<J, 1>(src, est, index, n_eff, M, N, ws, crit, singular, st);
    case 2: return gain_launch<J, 2>(src, est, index, n_eff, M, N, ws, crit, singular, st);
    case 3: return gain_launch<J, 3>(src, est, index, n_eff, M, N, ws, crit, singular, st);
    default: return gain_launch<J, 4>(src, est, index, n_eff, M, N, ws, crit, singular, st);
  }
}

__global__ void zero_int_kernel(int* p) { p[0] = 0; }

constexpr int kAsmThreads = 256;

__global__ __launch_bounds__(kAsmThreads) void te_assemble_kernel(const float* __restrict__ srcs,
                                                                  const int* __restrict__ lengths,
                                                                  const float* __restrict__ bgd, int S, int N,
                                                                  int spk_num, int nblk, float* __restrict__ mix,
                                                                  float* __restrict__ noise,
                                                                  float* __restrict__ target,
                                                                  int* __restrict__ mix_len) {
  const long long blk = blockIdx.x;
  const long long b = blk / nblk;
  const int x = (int)(blk % nblk);
  const long long i = (long long)x * kAsmThreads + threadIdx.x;
  if (x == 0 && threadIdx.x == 0 && mix_len) {
    int len = 0;
    for (int k = 0; k < spk_num; ++k) {
      int l = lengths ? lengths[b * S + k] : N;
      l = l < 0 ? 0 : (l > N ? N : l);
      len = l > len ? l : len;
    }
    mix_len[b] = len;
  }
  if (i >= N) return;
  const float* s = srcs + b * S * N + i;
  const float s0 = s[0];
  float m = s0 + s[N];  // (s_0 + s_1), then one add per further source: the reference's order
  float nz = s[N];
  for (int k = 2; k < spk_num; ++k) {
    const float v = s[(long long)k * N];
    m = m + v;
    nz = nz + v;
  }
  if (bgd) {
    const float g = bgd[i];
    m = m + g;
    nz = nz + g;
  }
  mix[b * N + i] = m;
  noise[b * N + i] = nz;
  target[b * N + i] = s0;
}

// [p, p + n) and [q, q + m) (bytes) overlap
inline bool overlaps(const void* p, long long n, const void* q, long long m) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

}  // namespace

DL4SS_API long long dl4ss_bss_gain_ws_bytes(int M, int N) {
  if (M < 0 || N < 1) return -1;
  return (long long)M * (gain_nchunk(N) * (kP1 + kP2) + DL4SS_BSS_GAIN_MAX_SRC * kCoef) * (long long)sizeof(double);
}

DL4SS_API int dl4ss_bss_gain(const float* src, const float* est, const int* index, const int* n_eff, int M, int J,
                             int Ke, int N, void* ws, long long ws_bytes, double* crit, int* singular,
                             void* stream) {
  DL4SS_REQUIRE(J >= 1 && J <= DL4SS_BSS_GAIN_MAX_SRC && Ke >= 1 && Ke <= DL4SS_BSS_GAIN_MAX_SRC);
  DL4SS_REQUIRE(N >= 1 && M >= 0);
  DL4SS_REQUIRE(src && est && index && crit && singular);
  GainIndex idx = {{0, 0, 0, 0}};
  for (int e = 0; e < Ke; ++e) {
    DL4SS_REQUIRE(index[e] >= 0 && index[e] < J);
    idx.v[e] = index[e];
  }
  const long long need = dl4ss_bss_gain_ws_bytes(M, N);
  DL4SS_REQUIRE((long long)M * gain_nchunk(N) <= 0x7FFFFFFFLL);
  hipStream_t st = as_stream(stream);
  if (M == 0) {
    hipLaunchKernelGGL(zero_int_kernel, dim3(1), dim3(1), 0, st, singular);
    DL4SS_CHECK_LAUNCH();
    return 0;
  }
  DL4SS_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0);
  double* w = static_cast<double*>(ws);
  switch (J) {
    case 1: return gain_launch_j<1>(Ke, src, est, idx, n_eff, M, N, w, crit, singular, st);
    case 2: return gain_launch_j<2>(Ke, src, est, idx, n_eff, M, N, w, crit, singular, st);
    case 3: return gain_launch_j<3>(Ke, src, est, idx, n_eff, M, N, w, crit, singular, st);
    default: return gain_launch_j<4>(Ke, src, est, idx, n_eff, M, N, w, crit, singular, st);
  }
}

DL4SS_API int dl4ss_te_assemble(const float* srcs, const int* lengths, const float* bgd, int B, int S, int N,
                                int spk_num, float* mix, float* noise, float* target, int* mix_len, void* stream) {
  DL4SS_REQUIRE(srcs && mix && noise && target);
  DL4SS_REQUIRE(B >= 0 && N >= 1 && S >= 2 && S <= 16 && spk_num >= 2 && spk_num <= S);
  const long long in_bytes = (long long)B * S * N * 4, out_bytes = (long long)B * N * 4;
  float* outs[3] = {mix, noise, target};
  for (int i = 0; i < 3; ++i) {
    DL4SS_REQUIRE(!overlaps(outs[i], out_bytes, srcs, in_bytes));
    DL4SS_REQUIRE(!(bgd && overlaps(outs[i], out_bytes, bgd, (long long)N * 4)));
    for (int j = i + 1; j < 3; ++j) DL4SS_REQUIRE(!overlaps(outs[i], out_bytes, outs[j], out_bytes));
  }
  if (B == 0) return 0;
  const int nblk = (int)cdiv(N, kAsmThreads);
  DL4SS_REQUIRE((long long)B * nblk <= 0x7FFFFFFFLL);
  hipLaunchKernelGGL(te_assemble_kernel, dim3((unsigned)((long long)B * nblk)), dim3(kAsmThreads), 0,
                     as_stream(stream), srcs, lengths, bgd, S, N, spk_num, nblk, mix, noise, target, mix_len);
  DL4SS_CHECK_LAUNCH();
  return 0;
}
