// Voiceprint path: a speaker is enrolled from clean speech (Cocktail/software/DL4SS_Keras/nnet.py:64-92).
//   - frame mask + compaction of the valid frames to a prefix (Masking / MaskingGt, nnet.py:44-47)
//   - row shifts that right-align the reverse direction of a variable-length batch, so that the
//     full-length recurrence kernels run each utterance's reverse pass from its own last frame
//   - the masked mean over an utterance's own frames (MeanPool, extend_layers.py:105-125)
//   - the life-long speaker memory (SpkLifeLongMemory / SelectSpkMemory / update_memory,
//     extend_layers.py:132-228)
// No atomics anywhere: every element has one owner and every sum a fixed order.
#include "common.h"

namespace {

constexpr int VP_TMAX = 2048;                    // frames per utterance the compaction stages in LDS
constexpr float VP_EPS = 2.220446049250313e-16f;  // np.spacing(1)

__device__ __forceinline__ int vp_len(const int* __restrict__ len, int b, int T) { return min(max(len[b], 0), T); }

// One workgroup per utterance: the frame mask (one wave per frame, 4 frames in flight), a serial scan
// over the <= 2048 flags by thread 0, then the gather of the valid rows.
__global__ __launch_bounds__(256) void vp_compact_kernel(const float* __restrict__ x, int T, int F, int rule,
                                                         float thr, const int* __restrict__ len_in,
                                                         float* __restrict__ xc, int* __restrict__ len,
                                                         int* __restrict__ idx) {
  __shared__ int sval[VP_TMAX];
  __shared__ int sidx[VP_TMAX];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* xb = x + (long long)b * T * F;
  if (len_in) {
    const int L = vp_len(len_in, b, T);
    for (int t = tid; t < T; t += 256) sval[t] = t < L;
  } else {
    for (int t = wave; t < T; t += 4) {  // wave-uniform
      bool hit = false;
      for (int f = lane; f < F; f += 64) {
        const float v = xb[(long long)t * F + f];
        hit |= rule == 0 ? v != 0.f : v > thr;
      }
      const bool any = __any(hit);
      if (lane == 0) sval[t] = any;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int t = 0; t < T; ++t)
      if (sval[t]) sidx[c++] = t;
    len[b] = c;
    for (; c < T; ++c) sidx[c] = -1;
  }
  __syncthreads();
  for (int j = tid; j < T; j += 256) idx[(long long)b * T + j] = sidx[j];
  float* xcb = xc + (long long)b * T * F;
  for (int i = tid; i < T * F; i += 256) {
    const int j = i / F, f = i - j * F;
    const int s = sidx[j];
    xcb[i] = s >= 0 ? xb[(long long)s * F + f] : 0.f;
  }
}

// dst[b, t, c] for c in [c0, c1): src's row t - d (dir > 0, rows < d zero) or t + d (dir < 0, rows >= len zero),
// d = T - len[b].  The other columns: other 0 untouched, 1 src where t < len and zero beyond, 2 src.
__global__ __launch_bounds__(256) void vp_shift_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                       long long total, int T, int ld, int c0, int c1,
                                                       const int* __restrict__ len, int dir, int other) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % ld);
  const long long r = i / ld;
  const int t = (int)(r % T), b = (int)(r / T);
  const int L = vp_len(len, b, T), d = T - L;
  if (c >= c0 && c < c1) {
    const int ts = dir > 0 ? t - d : t + d;
    const bool ok = dir > 0 ? t >= d : t < L;
    dst[i] = ok ? src[((long long)b * T + ts) * ld + c] : 0.f;
  } else if (other == 1) {
    dst[i] = t < L ? src[i] : 0.f;
  } else if (other == 2) {
    dst[i] = src[i];
  }
}

// vec[b, c] = sum over the utterance's own frames of out[b, t, c] / (len + eps), ascending t: the forward half
// (c < H) over rows [0, len), the reverse half over rows [T - len, T) (the recurrence kernel's frame).
__global__ __launch_bounds__(64) void vp_mean_fwd_kernel(const float* __restrict__ out, int T, int H,
                                                         const int* __restrict__ len, float* __restrict__ vec) {
  const int b = blockIdx.x, c = blockIdx.y * 64 + threadIdx.x;
  if (c >= 2 * H) return;
  const int L = vp_len(len, b, T);
  const int t0 = c < H ? 0 : T - L;
  const float* o = out + ((long long)b * T + t0) * 2 * H + c;
  float s = 0.f;
  for (int t = 0; t < L; ++t) s += o[(long long)t * 2 * H];
  vec[(long long)b * 2 * H + c] = s / ((float)L + VP_EPS);
}

// Every element of dOut (n, T, 2H) written: dvec / (len + eps) on the rows the mean read, zero elsewhere.
__global__ __launch_bounds__(256) void vp_mean_bwd_kernel(const float* __restrict__ dvec, long long total, int T,
                                                          int H, const int* __restrict__ len,
                                                          float* __restrict__ dOut) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % (2 * H));
  const long long r = i / (2 * H);
  const int t = (int)(r % T), b = (int)(r / T);
  const int L = vp_len(len, b, T);
  const bool valid = c < H ? t < L : t >= T - L;
  dOut[i] = valid ? dvec[(long long)b * 2 * H + c] / ((float)L + VP_EPS) : 0.f;
}

// ---- column sum in a fixed order for any row count (the bias gradient: colsum(dG)) ----
// Stage 1: block (x, p) sums rows [p * VP_CS_ROWS, ...) of 256 columns in ascending row, one thread a column,
// into part[p, c].  Stage 2: out[c] = sum over p of part[p, c] in ascending p.  The same M gives the same bits.
constexpr int VP_CS_ROWS = 64;

__global__ __launch_bounds__(256) void vp_colsum_part_kernel(const float* __restrict__ A, long long M, int C,
                                                             float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const long long r0 = (long long)blockIdx.y * VP_CS_ROWS;
  const long long r1 = r0 + VP_CS_ROWS < M ? r0 + VP_CS_ROWS : M;
  float s = 0.f;
  for (long long r = r0; r < r1; ++r) s += A[r * C + c];
  part[(long long)blockIdx.y * C + c] = s;
}

__global__ __launch_bounds__(256) void vp_colsum_final_kernel(const float* __restrict__ part, int P, int C,
                                                              float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += part[(long long)p * C + c];
  out[c] = s;
}

// ---- speaker memory: one workgroup of 4 waves, a wave per row, lane e owns columns e and e + 64 ----
// sqrt(sum_e w_e^2), w = a with eps where a == 0 (the reference's switch(eq(x, 0), eps, x))
__device__ __forceinline__ float vp_norm(float a0, float a1, int E, int lane) {
  const float w0 = lane < E ? (a0 == 0.f ? VP_EPS : a0) : 0.f;
  const float w1 = lane + 64 < E ? (a1 == 0.f ? VP_EPS : a1) : 0.f;
  return sqrtf(wave_sum(w0 * w0 + w1 * w1));
}

// r (+)= sum over the batch rows j with ids[j] == id of src[j], ascending j (wave-uniform walk)
__device__ __forceinline__ void vp_row_sum(const float* src, const int* __restrict__ ids, int n, int E, int id,
                                           int lane, float& r0, float& r1) {
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int jj = j0 + lane;
    unsigned long long m = __ballot(jj < n && ids[jj] == id);
    while (m) {
      const int j = j0 + __builtin_ctzll(m);
      m &= m - 1;
      if (lane < E) r0 += src[(long long)j * E + lane];
      if (lane + 64 < E) r1 += src[(long long)j * E + lane + 64];
    }
  }
}

__global__ __launch_bounds__(256) void spk_memory_fwd_kernel(const float* __restrict__ v,
                                                             const int* __restrict__ ids,
                                                             const float* __restrict__ mem, int n, int E, int M,
                                                             float* u, float* __restrict__ q) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < n; i += 4) {  // u_i = v_i / |w_i|
    const float v0 = lane < E ? v[(long long)i * E + lane] : 0.f;
    const float v1 = lane + 64 < E ? v[(long long)i * E + lane + 64] : 0.f;
    const float nrm = vp_norm(v0, v1, E, lane);
    if (lane < E) u[(long long)i * E + lane] = v0 / nrm;
    if (lane + 64 < E) u[(long long)i * E + lane + 64] = v1 / nrm;
  }
  __threadfence_block();
  __syncthreads();
  for (int i = wave; i < n; i += 4) {
    const int id = ids[i];
    float q0 = 0.f, q1 = 0.f;
    if (id >= 0 && id < M) {  // wave-uniform
      float a0 = lane < E ? mem[(long long)id * E + lane] : 0.f;
      float a1 = lane + 64 < E ? mem[(long long)id * E + lane + 64] : 0.f;
      vp_row_sum(u, ids, n, E, id, lane, a0, a1);
      const float nrm = vp_norm(a0, a1, E, lane);
      q0 = a0 / nrm;
      q1 = a1 / nrm;
    }
    if (lane < E) q[(long long)i * E + lane] = q0;
    if (lane + 64 < E) q[(long long)i * E + lane + 64] = q1;
  }
}

// dq -> dv through the gather, the row normalisation, the accumulation and the vector normalisation.
// For y = a / |w(a)|: da = g / N - ((g . a) / N) (a / N) / N  (the switch passes nothing to its constant
// branch, and a_e = 0 there anyway); the quotients are taken one at a time so that the projection term of an
// all-zero row (N ~ 1.5e-15) is 0, not 0 / 0.  The g / N term stays: an all-zero v gets the true derivative of
// v / |w|, of the order of 1e14 * g.  The trainer never sees it (vp_mean_bwd gives a len = 0 utterance a zero
// dOut); a caller that feeds a zero voiceprint from elsewhere does.
__global__ __launch_bounds__(256) void spk_memory_bwd_kernel(const float* __restrict__ dq,
                                                             const float* __restrict__ v,
                                                             const float* __restrict__ u,
                                                             const int* __restrict__ ids,
                                                             const float* __restrict__ mem, int n, int E, int M,
                                                             float* __restrict__ dv) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < n; i += 4) {
    const int id = ids[i];
    float d0 = 0.f, d1 = 0.f;
    if (id >= 0 && id < M) {
      float a0 = lane < E ? mem[(long long)id * E + lane] : 0.f;
      float a1 = lane + 64 < E ? mem[(long long)id * E + lane + 64] : 0.f;
      vp_row_sum(u, ids, n, E, id, lane, a0, a1);
      const float N = vp_norm(a0, a1, E, lane);
      float g0 = 0.f, g1 = 0.f;
      vp_row_sum(dq, ids, n, E, id, lane, g0, g1);
      const float ga = wave_sum(g0 * a0 + g1 * a1);
      const float dA0 = g0 / N - ((ga / N) * (a0 / N)) / N;
      const float dA1 = g1 / N - ((ga / N) * (a1 / N)) / N;
      const float v0 = lane < E ? v[(long long)i * E + lane] : 0.f;
      const float v1 = lane + 64 < E ? v[(long long)i * E + lane + 64] : 0.f;
      const float nv = vp_norm(v0, v1, E, lane);
      const float dv_ = wave_sum(dA0 * v0 + dA1 * v1);
      d0 = dA0 / nv - ((dv_ / nv) * (v0 / nv)) / nv;
      d1 = dA1 / nv - ((dv_ / nv) * (v1 / nv)) / nv;
    }
    if (lane < E) dv[(long long)i * E + lane] = d0;
    if (lane + 64 < E) dv[(long long)i * E + lane + 64] = d1;
  }
}

// mem[ids[i]] = q_i (duplicates carry identical rows); nothing when status[0] != 0 (a refused step)
__global__ __launch_bounds__(256) void spk_memory_store_kernel(const float* __restrict__ q,
                                                               const int* __restrict__ ids, int n, int E, int M,
                                                               float* __restrict__ mem,
                                                               const int* __restrict__ status) {
  if (status && status[0] != 0) return;
  const int i = blockIdx.x;
  const int id = ids[i];
  if (id < 0 || id >= M) return;
  for (int e = threadIdx.x; e < E; e += 256) mem[(long long)id * E + e] = q[(long long)i * E + e];
}

}  // namespace

DL4SS_API int dl4ss_vp_compact(const float* x, int n, int T, int F, int rule, float thr, const int* len_in,
                               float* xc, int* len, int* idx, void* stream) {
  DL4SS_REQUIRE(x && xc && len && idx && x != xc);
  DL4SS_REQUIRE(n >= 0 && n <= 65535 && T >= 1 && T <= VP_TMAX && F >= 1 && F <= 65536);
  DL4SS_REQUIRE(rule == 0 || rule == 1);
  DL4SS_REQUIRE(thr == thr);
  if (n == 0) return 0;
  hipLaunchKernelGGL(vp_compact_kernel, dim3(n), dim3(256), 0, as_stream(stream), x, T, F, rule, thr, len_in, xc,
                     len, idx);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_vp_shift(const float* src, float* dst, int n, int T, int ld, int c0, int c1, const int* len,
                             int dir, int other, void* stream) {
  DL4SS_REQUIRE(src && dst && len && src != dst);
  DL4SS_REQUIRE(n >= 0 && T >= 1 && ld >= 1 && 0 <= c0 && c0 <= c1 && c1 <= ld);
  DL4SS_REQUIRE(dir == 1 || dir == -1);
  DL4SS_REQUIRE(other >= 0 && other <= 2);
  const long long total = (long long)n * T * ld;
  DL4SS_REQUIRE(total <= 256LL * 0x7FFFFFFF);
  if (total == 0) return 0;
  hipLaunchKernelGGL(vp_shift_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), src, dst, total, T,
                     ld, c0, c1, len, dir, other);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_vp_mean_fwd(const float* out, int n, int T, int H, const int* len, float* vec, void* stream) {
  DL4SS_REQUIRE(out && len && vec);
  DL4SS_REQUIRE(n >= 0 && n <= 0x7FFFFFFF && T >= 1 && H >= 1 && H <= (1 << 20));
  if (n == 0) return 0;
  hipLaunchKernelGGL(vp_mean_fwd_kernel, dim3(n, cdiv(2 * H, 64)), dim3(64), 0, as_stream(stream), out, T, H, len,
                     vec);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_vp_mean_bwd(const float* dvec, int n, int T, int H, const int* len, float* dOut, void* stream) {
  DL4SS_REQUIRE(dvec && len && dOut);
  DL4SS_REQUIRE(n >= 0 && T >= 1 && H >= 1 && H <= (1 << 20));
  const long long total = (long long)n * T * 2 * H;
  DL4SS_REQUIRE(total <= 256LL * 0x7FFFFFFF);
  if (total == 0) return 0;
  hipLaunchKernelGGL(vp_mean_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), dvec, total, T,
                     H, len, dOut);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API long long dl4ss_vp_colsum_parts(long long M) {
  return M < 1 || M > 65535LL * VP_CS_ROWS ? -1 : (M + VP_CS_ROWS - 1) / VP_CS_ROWS;
}

DL4SS_API int dl4ss_vp_colsum(const float* A, long long M, int C, float* part, float* out, void* stream) {
  DL4SS_REQUIRE(A && part && out && part != A && out != A && out != part);
  DL4SS_REQUIRE(M >= 1 && M <= 65535LL * VP_CS_ROWS && C >= 1 && C <= (1 << 20));
  const long long P = (M + VP_CS_ROWS - 1) / VP_CS_ROWS;
  hipLaunchKernelGGL(vp_colsum_part_kernel, dim3(cdiv(C, 256), (unsigned)P), dim3(256), 0, as_stream(stream), A, M,
                     C, part);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL(vp_colsum_final_kernel, dim3(cdiv(C, 256)), dim3(256), 0, as_stream(stream), part, (int)P, C,
                     out);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_spk_memory_fwd(const float* v, const int* ids, const float* mem, int n, int E, int M, float* u,
                                   float* q, void* stream) {
  DL4SS_REQUIRE(v && ids && mem && u && q && u != v && q != v && q != u);
  DL4SS_REQUIRE(n >= 0 && n <= 1024 && E >= 1 && E <= 128 && M >= 1);
  if (n == 0) return 0;
  hipLaunchKernelGGL(spk_memory_fwd_kernel, dim3(1), dim3(256), 0, as_stream(stream), v, ids, mem, n, E, M, u, q);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_spk_memory_bwd(const float* dq, const float* v, const float* u, const int* ids,
                                   const float* mem, int n, int E, int M, float* dv, void* stream) {
  DL4SS_REQUIRE(dq && v && u && ids && mem && dv && dv != dq && dv != v && dv != u);
  DL4SS_REQUIRE(n >= 0 && n <= 1024 && E >= 1 && E <= 128 && M >= 1);
  if (n == 0) return 0;
  hipLaunchKernelGGL(spk_memory_bwd_kernel, dim3(1), dim3(256), 0, as_stream(stream), dq, v, u, ids, mem, n, E, M,
                     dv);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_spk_memory_store(const float* q, const int* ids, int n, int E, int M, float* mem,
                                     const int* status, void* stream) {
  DL4SS_REQUIRE(q && ids && mem && q != mem);
  DL4SS_REQUIRE(n >= 0 && n <= 1024 && E >= 1 && E <= 128 && M >= 1);
  if (n == 0) return 0;
  hipLaunchKernelGGL(spk_memory_store_kernel, dim3(n), dim3(256), 0, as_stream(stream), q, ids, n, E, M, mem,
                     status);
  DL4SS_CHECK_LAUNCH();
  return 0;
}
