// Image query: the target is named by a picture (Multi_modal/software/DL4SS_Keras/nnet.py:70-89).  A small CNN
// (three conv + ReLU + 2x2 max-pool stages and a dense layer: include/dl4ss_imgq.h has the table and the
// parameter layout) turns an image into the vector the speaker memory accumulates.  ~0.1 MFLOP an image: one
// fused kernel per direction, one workgroup per image, every activation in LDS, fp32 VALU throughout.
//
// What a stage keeps per pooled cell is its value and a code: the window position (row-major 0..3) of the first
// maximum of the four pre-activations, or -1 when that maximum is <= 0 (ReLU dead: pool(relu(z)) then passes no
// gradient whichever element the pool picks).  The pre-activations themselves are never stored, so the gradient
// at a stage's pre-activations is one value per pooled cell, at the coded position.
//
// LDS banks (ds_read_b32: bank = dword address % 32, conflicts within each 32-lane half): consecutive lanes own
// consecutive pooled columns of one channel, so a lane's window reads are 2 dwords from its neighbour's: lanes
// l and l + 16 meet on a bank, 2-way.  A stride-1 mapping (a lane per pre-activation, pooled in a second pass)
// is conflict free but needs the pre-activations in LDS (4x the pooled map) and a barrier more per stage; the
// weights are one address per channel, a broadcast.  The whole forward is ~100 k FMAs on one CU, latency bound
// at 2-way or not, so the smaller plan is taken.
// No atomics: every output element has one owner and every sum a fixed order.
#include "common.h"

#include "../../include/dl4ss_imgq.h"

namespace {

constexpr int IQ_THREADS = 256;

struct IqDims {
  int h, w, h1, w1, h2, w2, h3, w3, E, D;
  // LDS plan, float offsets: image, pooled maps p1..p3, gradient maps g1..g3, conv parameters, dvec; then the
  // codes a1..a3 as bytes behind the floats
  int o_img, o_p1, o_p2, o_p3, o_g1, o_g2, o_g3, o_par, o_dv, n_float;
  int o_a1, o_a2, o_a3, n_code;
};

inline bool iq_dims(int h, int w, int E, IqDims& d) {
  if (h < DL4SS_IMGQ_MIN_HW || h > DL4SS_IMGQ_MAX_HW || w < DL4SS_IMGQ_MIN_HW || w > DL4SS_IMGQ_MAX_HW) return false;
  if (E < 1 || E > DL4SS_IMGQ_MAX_E) return false;
  d.h = h, d.w = w, d.E = E;
  d.h1 = (h - 4) / 2, d.w1 = (w - 4) / 2;
  d.h2 = (d.h1 - 2) / 2, d.w2 = (d.w1 - 2) / 2;
  d.h3 = (d.h2 - 2) / 2, d.w3 = (d.w2 - 2) / 2;
  d.D = 16 * d.h3 * d.w3;
  const int n1 = 4 * d.h1 * d.w1, n2 = 8 * d.h2 * d.w2, n3 = d.D;
  int o = 0;
  d.o_img = o, o += h * w;
  d.o_p1 = o, o += n1;
  d.o_p2 = o, o += n2;
  d.o_p3 = o, o += n3;
  d.o_g1 = o, o += n1;
  d.o_g2 = o, o += n2;
  d.o_g3 = o, o += n3;
  d.o_par = o, o += DL4SS_IMGQ_CONV_PARAMS;
  d.o_dv = o, o += DL4SS_IMGQ_MAX_E;
  d.n_float = o;
  d.o_a1 = 0, d.o_a2 = n1, d.o_a3 = n1 + n2;
  d.n_code = n1 + n2 + n3;
  return true;
}

inline size_t iq_lds_bytes(const IqDims& d) { return (size_t)d.n_float * 4 + (size_t)((d.n_code + 3) / 4 * 4); }

// One stage: out (CO, ph, pw) = pool2x2(relu(conv KSxKS valid(in (CI, hin, win)) + bias)), ph = (hin - KS + 1) / 2;
// code as above.  A thread per pooled cell; the sum runs over (ci, ky, kx) ascending from the bias.
template <int CI, int CO, int KS>
__device__ __forceinline__ void iq_stage(const float* in, int hin, int win, const float* W, const float* bias,
                                         float* out, signed char* code, int ph, int pw, int tid) {
  const int cells = ph * pw;
  for (int i = tid; i < CO * cells; i += IQ_THREADS) {
    const int co = i / cells, c = i - co * cells;
    const int py = c / pw, px = c - py * pw;
    const float b = bias[co];
    float z00 = b, z01 = b, z10 = b, z11 = b;
    for (int ci = 0; ci < CI; ++ci) {
      const float* ip = in + (ci * hin + 2 * py) * win + 2 * px;
      const float* wp = W + (co * CI + ci) * KS * KS;
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
          const float wv = wp[ky * KS + kx];
          z00 = fmaf(wv, ip[ky * win + kx], z00);
          z01 = fmaf(wv, ip[ky * win + kx + 1], z01);
          z10 = fmaf(wv, ip[(ky + 1) * win + kx], z10);
          z11 = fmaf(wv, ip[(ky + 1) * win + kx + 1], z11);
        }
      }
    }
    float m = z00;
    int a = 0;
    if (z01 > m) m = z01, a = 1;  // strictly greater: the first maximum stays
    if (z10 > m) m = z10, a = 2;
    if (z11 > m) m = z11, a = 3;
    out[i] = m > 0.f ? m : 0.f;
    code[i] = (signed char)(m > 0.f ? a : -1);
  }
}

// The image and the convolution parameters into LDS, then the three stages.  Ends behind a barrier.
__device__ __forceinline__ void iq_forward(const IqDims& d, const float* __restrict__ img,
                                           const float* __restrict__ params, float* sm, signed char* sc, int tid) {
  float* par = sm + d.o_par;
  for (int i = tid; i < d.h * d.w; i += IQ_THREADS) sm[d.o_img + i] = img[i];
  for (int i = tid; i < DL4SS_IMGQ_CONV_PARAMS; i += IQ_THREADS) par[i] = params[i];
  __syncthreads();
  iq_stage<1, 4, 5>(sm + d.o_img, d.h, d.w, par + DL4SS_IMGQ_OFF_W1, par + DL4SS_IMGQ_OFF_B1, sm + d.o_p1,
                    sc + d.o_a1, d.h1, d.w1, tid);
  __syncthreads();
  iq_stage<4, 8, 3>(sm + d.o_p1, d.h1, d.w1, par + DL4SS_IMGQ_OFF_W2, par + DL4SS_IMGQ_OFF_B2, sm + d.o_p2,
                    sc + d.o_a2, d.h2, d.w2, tid);
  __syncthreads();
  iq_stage<8, 16, 3>(sm + d.o_p2, d.h2, d.w2, par + DL4SS_IMGQ_OFF_W3, par + DL4SS_IMGQ_OFF_B3, sm + d.o_p3,
                     sc + d.o_a3, d.h3, d.w3, tid);
  __syncthreads();
}

// vec[e] = dense.bias[e] + dense.weight[e] . p3: a wave per output, lane l sums the inputs l, l + 64, ... in
// ascending order, then the butterfly.  dense.weight is read from global memory, each element once an image
// (E D floats, up to 128 KB: it stays out of the LDS plan).
__global__ __launch_bounds__(IQ_THREADS) void imgq_fwd_kernel(IqDims d, const float* __restrict__ images,
                                                              const float* __restrict__ params,
                                                              float* __restrict__ vec) {
  extern __shared__ float sm[];
  signed char* sc = reinterpret_cast<signed char*>(sm + d.n_float);
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  iq_forward(d, images + (long long)b * d.h * d.w, params, sm, sc, tid);
  const float* p3 = sm + d.o_p3;
  const float* Wd = params + DL4SS_IMGQ_OFF_WD;
  const float* bd = Wd + (long long)d.E * d.D;
  for (int e = wave; e < d.E; e += IQ_THREADS / 64) {  // wave-uniform
    float s = 0.f;
    for (int i = lane; i < d.D; i += 64) s = fmaf(Wd[(long long)e * d.D + i], p3[i], s);
    s = wave_sum(s);
    if (lane == 0) vec[(long long)b * d.E + e] = s + bd[e];
  }
}

// dW[co, ci, ky, kx] = sum over the pooled cells, row-major ascending, of g[co, cell] x the input under the
// cell's coded pre-activation; a thread per weight.  (g is zero at dead cells; they are skipped.)
template <int CI, int CO, int KS>
__device__ __forceinline__ void iq_wgrad(const float* in, int hin, int win, const float* g, const signed char* code,
                                         int ph, int pw, float* __restrict__ dW, int tid) {
  for (int i = tid; i < CO * CI * KS * KS; i += IQ_THREADS) {
    const int kx = i % KS, ky = (i / KS) % KS, ci = (i / (KS * KS)) % CI, co = i / (KS * KS * CI);
    const float* ip = in + (ci * hin + ky) * win + kx;
    const float* gp = g + co * ph * pw;
    const signed char* cp = code + co * ph * pw;
    float s = 0.f;
    for (int py = 0; py < ph; ++py)
      for (int px = 0; px < pw; ++px) {
        const int a = cp[py * pw + px];
        if (a >= 0) s = fmaf(gp[py * pw + px], ip[(2 * py + (a >> 1)) * win + 2 * px + (a & 1)], s);
      }
    dW[i] = s;
  }
}

// db[co] = sum of g[co, :]: a wave per channel, lane l the cells l, l + 64, ... ascending, then the butterfly.
template <int CO>
__device__ __forceinline__ void iq_bgrad(const float* g, int cells, float* __restrict__ db, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  for (int co = wave; co < CO; co += IQ_THREADS / 64) {
    float s = 0.f;
    for (int c = lane; c < cells; c += 64) s += g[co * cells + c];
    s = wave_sum(s);
    if (lane == 0) db[co] = s;
  }
}

// The gradient at the stage's input map (CI, hin, win), masked by that map's own codes (it is the pooled output
// of the stage below): gin[ci, y, x] = sum over (co, ky, kx) ascending of g[co, cell] W[co, ci, ky, kx] where the
// pre-activation (y - ky, x - kx) is the coded one of its cell.  A gather, a thread per input element.
template <int CI, int CO, int KS>
__device__ __forceinline__ void iq_dgrad(const float* g, const signed char* code, int ph, int pw, const float* W,
                                         const signed char* code_in, int hin, int win, float* gin, int tid) {
  for (int i = tid; i < CI * hin * win; i += IQ_THREADS) {
    float s = 0.f;
    if (code_in[i] >= 0) {
      const int x = i % win, y = (i / win) % hin, ci = i / (win * hin);
      for (int co = 0; co < CO; ++co) {
        const float* wp = W + (co * CI + ci) * KS * KS;
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
          const int oy = y - ky;
          if (oy < 0 || oy >= 2 * ph) continue;
#pragma unroll
          for (int kx = 0; kx < KS; ++kx) {
            const int ox = x - kx;
            if (ox < 0 || ox >= 2 * pw) continue;
            const int c = co * ph * pw + (oy >> 1) * pw + (ox >> 1);
            if (code[c] == (oy & 1) * 2 + (ox & 1)) s = fmaf(g[c], wp[ky * KS + kx], s);
          }
        }
      }
    }
    gin[i] = s;
  }
}

__global__ __launch_bounds__(IQ_THREADS) void imgq_bwd_kernel(IqDims d, const float* __restrict__ images,
                                                              const float* __restrict__ dvec,
                                                              const float* __restrict__ params, int P,
                                                              long long ld, float* __restrict__ dpart) {
  extern __shared__ float sm[];
  signed char* sc = reinterpret_cast<signed char*>(sm + d.n_float);
  const int b = blockIdx.x, tid = threadIdx.x;
  float* dv = sm + d.o_dv;
  for (int e = tid; e < d.E; e += IQ_THREADS) dv[e] = dvec[(long long)b * d.E + e];
  iq_forward(d, images + (long long)b * d.h * d.w, params, sm, sc, tid);  // (its barriers cover dv)
  float* row = dpart + (long long)b * ld;
  const float* par = sm + d.o_par;
  const float* p3 = sm + d.o_p3;
  const float* Wd = params + DL4SS_IMGQ_OFF_WD;
  const int E = d.E, D = d.D;
  // dense: dW = dvec (x) p3, db = dvec, and the gradient at the cells of stage 3
  for (int i = tid; i < E * D; i += IQ_THREADS) row[DL4SS_IMGQ_OFF_WD + i] = dv[i / D] * p3[i % D];
  for (int e = tid; e < E; e += IQ_THREADS) row[DL4SS_IMGQ_OFF_WD + E * D + e] = dv[e];
  for (long long i = P + tid; i < ld; i += IQ_THREADS) row[i] = 0.f;
  for (int i = tid; i < D; i += IQ_THREADS) {
    float s = 0.f;
    if (sc[d.o_a3 + i] >= 0)
      for (int e = 0; e < E; ++e) s = fmaf(dv[e], Wd[(long long)e * D + i], s);
    sm[d.o_g3 + i] = s;
  }
  __syncthreads();
  iq_wgrad<8, 16, 3>(sm + d.o_p2, d.h2, d.w2, sm + d.o_g3, sc + d.o_a3, d.h3, d.w3, row + DL4SS_IMGQ_OFF_W3, tid);
  iq_bgrad<16>(sm + d.o_g3, d.h3 * d.w3, row + DL4SS_IMGQ_OFF_B3, tid);
  iq_dgrad<8, 16, 3>(sm + d.o_g3, sc + d.o_a3, d.h3, d.w3, par + DL4SS_IMGQ_OFF_W3, sc + d.o_a2, d.h2, d.w2,
                     sm + d.o_g2, tid);
  __syncthreads();
  iq_wgrad<4, 8, 3>(sm + d.o_p1, d.h1, d.w1, sm + d.o_g2, sc + d.o_a2, d.h2, d.w2, row + DL4SS_IMGQ_OFF_W2, tid);
  iq_bgrad<8>(sm + d.o_g2, d.h2 * d.w2, row + DL4SS_IMGQ_OFF_B2, tid);
  iq_dgrad<4, 8, 3>(sm + d.o_g2, sc + d.o_a2, d.h2, d.w2, par + DL4SS_IMGQ_OFF_W2, sc + d.o_a1, d.h1, d.w1,
                    sm + d.o_g1, tid);
  __syncthreads();
  iq_wgrad<1, 4, 5>(sm + d.o_img, d.h, d.w, sm + d.o_g1, sc + d.o_a1, d.h1, d.w1, row + DL4SS_IMGQ_OFF_W1, tid);
  iq_bgrad<4>(sm + d.o_g1, d.h1 * d.w1, row + DL4SS_IMGQ_OFF_B1, tid);
}

// out[c] = sum over the n rows of dpart[:, c], pairwise in a fixed order: rows are taken in ascending order and
// two partial sums of 2^l consecutive rows each are added (earlier + later) as soon as both exist -- st[l] holds
// the pending sum of level l --, so the sum's rounding error grows with log2(n), not n; what is left at the end
// (the set bits of n) is folded from the latest rows back to the earliest.  A thread per column: the same n gives
// the same bits.  n <= 1024: 11 levels, statically indexed (registers).
constexpr int IQ_LEVELS = 11;

__global__ __launch_bounds__(IQ_THREADS) void imgq_reduce_kernel(const float* __restrict__ dpart, int n, long long ld,
                                                                 float* __restrict__ out) {
  const long long c = (long long)blockIdx.x * IQ_THREADS + threadIdx.x;
  if (c >= ld) return;
  float st[IQ_LEVELS];
#pragma unroll
  for (int l = 0; l < IQ_LEVELS; ++l) st[l] = 0.f;
  for (int i = 0; i < n; ++i) {
    float s = dpart[(long long)i * ld + c];
    int k = i + 1;
    bool placed = false;
#pragma unroll
    for (int l = 0; l < IQ_LEVELS; ++l) {
      if (!placed) {
        if (k & 1) {
          st[l] = s;
          placed = true;
        } else {
          s = st[l] + s;
          k >>= 1;
        }
      }
    }
  }
  float total = 0.f;
  bool have = false;
#pragma unroll
  for (int l = 0; l < IQ_LEVELS; ++l) {
    if ((n >> l) & 1) {
      total = have ? st[l] + total : st[l];
      have = true;
    }
  }
  out[c] = total;
}

__global__ void imgq_guard_kernel(const float* __restrict__ loss, int* __restrict__ status) {
  const float l = loss[0];
  if (threadIdx.x == 0 && !(fabsf(l) <= 3.4028234664e38f)) status[0] |= 2;
}

// [a, a + na) and [b, b + nb) floats overlap
inline bool iq_overlap(const float* a, long long na, const float* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

}  // namespace

DL4SS_API long long dl4ss_imgq_dense_in(int h, int w) {
  IqDims d;
  return iq_dims(h, w, 1, d) ? d.D : -1;
}

DL4SS_API long long dl4ss_imgq_param_count(int h, int w, int E) {
  IqDims d;
  return iq_dims(h, w, E, d) ? (long long)DL4SS_IMGQ_CONV_PARAMS + (long long)E * d.D + E : -1;
}

DL4SS_API int dl4ss_imgq_fwd(const float* images, const float* params, int n, int h, int w, int E, float* vec,
                             void* stream) {
  IqDims d;
  DL4SS_REQUIRE(images && params && vec);
  DL4SS_REQUIRE(n >= 0 && n <= DL4SS_IMGQ_MAX_N);
  DL4SS_REQUIRE(iq_dims(h, w, E, d));
  const long long P = dl4ss_imgq_param_count(h, w, E);
  DL4SS_REQUIRE(!iq_overlap(vec, (long long)n * E, images, (long long)n * h * w) && vec != images);
  DL4SS_REQUIRE(!iq_overlap(vec, (long long)n * E, params, P) && vec != params);
  if (n == 0) return 0;
  hipLaunchKernelGGL(imgq_fwd_kernel, dim3(n), dim3(IQ_THREADS), iq_lds_bytes(d), as_stream(stream), d, images,
                     params, vec);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_imgq_bwd(const float* images, const float* dvec, const float* params, int n, int h, int w, int E,
                             float* dpart, long long ld, long long dpart_floats, void* stream) {
  IqDims d;
  DL4SS_REQUIRE(images && dvec && params && dpart);
  DL4SS_REQUIRE(n >= 0 && n <= DL4SS_IMGQ_MAX_N);
  DL4SS_REQUIRE(iq_dims(h, w, E, d));
  const long long P = dl4ss_imgq_param_count(h, w, E);
  DL4SS_REQUIRE(ld >= P && ld <= (1 << 20));
  DL4SS_REQUIRE(dpart_floats >= (long long)n * ld);  // the workspace holds every row
  DL4SS_REQUIRE(dpart != images && dpart != dvec && dpart != params);
  DL4SS_REQUIRE(!iq_overlap(dpart, (long long)n * ld, images, (long long)n * h * w));
  DL4SS_REQUIRE(!iq_overlap(dpart, (long long)n * ld, dvec, (long long)n * E));
  DL4SS_REQUIRE(!iq_overlap(dpart, (long long)n * ld, params, P));
  if (n == 0) return 0;
  hipLaunchKernelGGL(imgq_bwd_kernel, dim3(n), dim3(IQ_THREADS), iq_lds_bytes(d), as_stream(stream), d, images,
                     dvec, params, (int)P, ld, dpart);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_imgq_reduce(const float* dpart, int n, long long ld, float* out, void* stream) {
  DL4SS_REQUIRE(dpart && out);
  DL4SS_REQUIRE(n >= 0 && n <= DL4SS_IMGQ_MAX_N && ld >= 1 && ld <= (1 << 20));
  DL4SS_REQUIRE(!iq_overlap(out, ld, dpart, (long long)n * ld) && out != dpart);
  if (n == 0) return 0;
  hipLaunchKernelGGL(imgq_reduce_kernel, dim3(cdiv(ld, IQ_THREADS)), dim3(IQ_THREADS), 0, as_stream(stream), dpart, n,
                     ld, out);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_imgq_guard(const float* loss, int* status, void* stream) {
  DL4SS_REQUIRE(loss && status);
  hipLaunchKernelGGL(imgq_guard_kernel, dim3(1), dim3(64), 0, as_stream(stream), loss, status);
  DL4SS_CHECK_LAUNCH();
  return 0;
}
