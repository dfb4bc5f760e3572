// The guarded parameter update shared by small.hip (the Adam entry points of dl4ss_hip.h) and optim.hip (Nadam and
// Keras's clipnorm, dl4ss_optim.h): the bf16 shadow stores, the fixed-order fp64 block sum, the one update kernel
// and its launcher.  Both files instantiate the kernel from this one text, so an instantiation they share
// (Adam with torch's clip) is the same code in both.
#pragma once
#include "common.h"

namespace {

// bf16 shadow copies written by the update (the bf16 step's GEMM / recurrence operands): segment s
// maps the flat range [off, off + rows*cols) row-major onto y[r * ldy + c] (columns >= cols untouched)
constexpr int SHADOW_MAX = 8;
struct ShadowSegs {
  long long off[SHADOW_MAX], len[SHADOW_MAX], ldy[SHADOW_MAX];
  int cols[SHADOW_MAX];
  unsigned short* y[SHADOW_MAX];
  int n;
};
__device__ __forceinline__ void shadow_store(const ShadowSegs& sh, long long i, float x) {
#pragma unroll
  for (int s = 0; s < SHADOW_MAX; ++s) {
    if (s >= sh.n) break;
    const long long j = i - sh.off[s];
    if (j >= 0 && j < sh.len[s]) {
      const unsigned r = (unsigned)j / (unsigned)sh.cols[s], c = (unsigned)j - r * (unsigned)sh.cols[s];
      sh.y[s][r * sh.ldy[s] + c] = (unsigned short)bf16_bits_rne(x);
      return;
    }
  }
}
// four consecutive flat elements i..i+3: one 8-B store when they sit in one row of one segment at
// an 8-B aligned destination (the 600-column weights: every quad), else element by element
__device__ __forceinline__ void shadow_store4(const ShadowSegs& sh, long long i, float4 x) {
#pragma unroll
  for (int s = 0; s < SHADOW_MAX; ++s) {
    if (s >= sh.n) break;
    const long long j = i - sh.off[s];
    if (j + 3 < 0 || j >= sh.len[s]) continue;
    if (j >= 0 && j + 3 < sh.len[s]) {
      const unsigned r = (unsigned)j / (unsigned)sh.cols[s], c = (unsigned)j - r * (unsigned)sh.cols[s];
      const long long o = r * sh.ldy[s] + c;
      if (c + 3 < (unsigned)sh.cols[s] && (o & 3) == 0) {
        const unsigned lo = bf16_bits_rne(x.x) | (bf16_bits_rne(x.y) << 16);
        const unsigned hi = bf16_bits_rne(x.z) | (bf16_bits_rne(x.w) << 16);
        *reinterpret_cast<uint2*>(sh.y[s] + o) = make_uint2(lo, hi);
        return;
      }
    }
    break;  // a quad across a row or segment boundary
  }
  shadow_store(sh, i, x.x); shadow_store(sh, i + 1, x.y); shadow_store(sh, i + 2, x.z); shadow_store(sh, i + 3, x.w);
}

// every thread of a 256-thread block gets the sum of the block's values (a fixed tree: butterfly inside
// each wave, then the four wave sums in wave order)
__device__ __forceinline__ double block_sum_d(double v, double* sd) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sd[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sd[0] + sd[1]) + sd[2]) + sd[3];
}

enum { UPD_ADAM = 0, UPD_NADAM = 1 };
// CLIP_TORCH: c = min(1, max_norm / (nrm + 1e-6)) (torch.nn.utils.clip_grad_norm_);
// CLIP_KERAS: c = max_norm / nrm where nrm >= max_norm, else 1 (Keras 1, Optimizer.get_gradients / clip_norm)
enum { CLIP_NONE = 0, CLIP_TORCH = 1, CLIP_KERAS = 2 };
constexpr int CLIP_MAX_PARTS = 4096;
constexpr int STATUS_NONFINITE_GRAD = 4;  // the sticky bit of status[0] (ClipArgs::sticky)

// the clipped update's extra arguments
struct ClipArgs {
  const double* part;  // fp64 partial sums of squares (grad_sumsq_kernel's, of one gradient or of several)
  int n_part;
  float max_norm;
  float* gnorm;        // [2]: the norm of the mean gradient before clipping, the coefficient c (may be NULL)
  int* nonfinite;      // [1]: updates refused for a non-finite gradient
  int sticky;          // non-zero: such a refusal also sets STATUS_NONFINITE_GRAD in status[0]
};

// KIND UPD_ADAM: torch.optim.Adam (weight_decay 0, amsgrad off; m via lerp as torch) on flat fp32 buffers
// (EvalVer.py:538-544,673-675: Adam(lr=2e-4), betas (0.9, 0.999), eps 1e-8).
// KIND UPD_NADAM: Keras 1's Nadam (DL4SS_Keras/nnet.py:23,113), the momentum schedule's scalars from the host:
//   gs = g f;  m' = b1 m + (1 - b1) gs;  v' = b2 v + (1 - b2) gs^2;
//   p' = p - (a1 gs + a2 m') / (sqrt(v') / bc2s + eps),   a1 = lr (1 - mu_t) / (1 - P_t),  a2 = lr mu_{t+1} / (1 - P_{t+1})
// (lr is then unused, bc1 too).  Every multiply-add of it is written as an explicit fmaf, so every instantiation
// rounds alike.
// SH: also the bf16 shadow copies of the updated parameters (bitwise dl4ss_f32_to_bf16_2d_multi of the new values).
// CLIP: the global-norm clip on the mean gradient, folded into gscale.  Every block sums the partials in the same
// fixed order (<= 32 KB from L2) and so forms the same factor, or takes the same refusal when the sum is not
// finite; without CLIP the code is the unclipped kernel's.
template <int KIND, int CLIP, bool SH>
__global__ __launch_bounds__(256) void update_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ v, long long n,
                                                     float lr, float b1, float b2, float eps, float bc1, float bc2s,
                                                     int* status, int* refused,
                                                     const float* __restrict__ dp_flag, float gscale,
                                                     float* __restrict__ loss, ShadowSegs sh, ClipArgs cl, float a1,
                                                     float a2) {
  // (status and refused are plain pointers: refused is status + 1, and the sticky bit is written through status)
  // refuse the update when a recurrence hand-off of this step timed out on this rank
  // (status[0]) or on any data-parallel peer (dp_flag: the all-reduced status flag)
  if ((status && status[0]) || (dp_flag && dp_flag[0] != 0.f)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (loss) loss[0] = __builtin_nanf("");
      if (refused) refused[0] += 1;  // refused-update count: the host rolls its step count back by it
    }
    return;
  }
  if constexpr (CLIP != CLIP_NONE) {
    __shared__ double sd[4];
    double s = 0.0;
    for (int j = threadIdx.x; j < cl.n_part; j += 256) s += cl.part[j];
    s = block_sum_d(s, sd);
    // fp64 throughout: nrm = ||g * gscale||, the coefficient c, one fp32 factor f = gscale c
    const double nrm = (double)gscale * sqrt(s);
    double c;
    if constexpr (CLIP == CLIP_TORCH) c = fmin(1.0, (double)cl.max_norm / (nrm + 1e-6));
    else c = nrm >= (double)cl.max_norm ? (double)cl.max_norm / nrm : 1.0;
    if (!isfinite(s)) {  // an Inf or NaN in the gradient: refused as a timed-out step is, and counted
      // (sticky: a block that reads the bit at its start takes the refusal above and returns as it would here;
      // the counts are this thread's alone, and it read status[0] before it writes)
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (loss) loss[0] = __builtin_nanf("");
        if (refused) refused[0] += 1;
        cl.nonfinite[0] += 1;
        if (cl.sticky && status) status[0] |= STATUS_NONFINITE_GRAD;
        if (cl.gnorm) { cl.gnorm[0] = (float)nrm; cl.gnorm[1] = 0.f; }
      }
      return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && cl.gnorm) { cl.gnorm[0] = (float)nrm; cl.gnorm[1] = (float)c; }
    gscale = (float)((double)gscale * c);  // c == 1: bitwise gscale
  }
  const float step = lr / bc1;
  const float omb1 = 1.f - b1, omb2 = 1.f - b2;
  for (long long i = (blockIdx.x * (long long)blockDim.x + threadIdx.x) * 4; i < n;
       i += (long long)gridDim.x * blockDim.x * 4) {
    if (i + 3 < n) {
      float4 pp = *reinterpret_cast<float4*>(p + i);
      float4 gg = *reinterpret_cast<const float4*>(g + i);
      gg.x *= gscale; gg.y *= gscale; gg.z *= gscale; gg.w *= gscale;  // 1 / world (DP SUM); 1: exact
      float4 mm = *reinterpret_cast<float4*>(m + i);
      float4 vv = *reinterpret_cast<float4*>(v + i);
      if constexpr (KIND == UPD_ADAM) {
#define ADAM1(c)                                              \
  mm.c = mm.c + (1.f - b1) * (gg.c - mm.c);                    \
  vv.c = b2 * vv.c + (1.f - b2) * gg.c * gg.c;                 \
  pp.c -= step * (mm.c / (sqrtf(vv.c) / bc2s + eps));
        ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
      } else {
#define NADAM1(c)                                                            \
  mm.c = fmaf(b1, mm.c, omb1 * gg.c);                                         \
  vv.c = fmaf(b2, vv.c, (omb2 * gg.c) * gg.c);                                \
  pp.c = pp.c - fmaf(a1, gg.c, a2 * mm.c) / (sqrtf(vv.c) / bc2s + eps);
        NADAM1(x) NADAM1(y) NADAM1(z) NADAM1(w)
#undef NADAM1
      }
      *reinterpret_cast<float4*>(p + i) = pp;
      *reinterpret_cast<float4*>(m + i) = mm;
      *reinterpret_cast<float4*>(v + i) = vv;
      if constexpr (SH) {
        shadow_store4(sh, i, pp);
      }
    } else {
      for (long long j = i; j < n; ++j) {
        const float gj = g[j] * gscale;
        if constexpr (KIND == UPD_ADAM) {
          m[j] = m[j] + (1.f - b1) * (gj - m[j]);
          v[j] = b2 * v[j] + (1.f - b2) * gj * gj;
          p[j] -= step * (m[j] / (sqrtf(v[j]) / bc2s + eps));
        } else {
          const float mj = fmaf(b1, m[j], omb1 * gj), vj = fmaf(b2, v[j], (omb2 * gj) * gj);
          m[j] = mj;
          v[j] = vj;
          p[j] = p[j] - fmaf(a1, gj, a2 * mj) / (sqrtf(vj) / bc2s + eps);
        }
        if constexpr (SH) shadow_store(sh, j, p[j]);
      }
    }
  }
}

// the scalars an update is launched with beside the hyper-parameters: Adam's bias corrections, or Nadam's a1, a2
struct UpdateScalars {
  int kind;
  float bc1, bc2s, a1, a2;
};
// bias corrections in double on the host, as torch computes them in Python floats
static inline UpdateScalars adam_scalars(float beta1, float beta2, int step) {
  return {UPD_ADAM, (float)(1.0 - pow((double)beta1, (double)step)),
          (float)sqrt(1.0 - pow((double)beta2, (double)step)), 0.f, 0.f};
}

static inline int update_launch(const UpdateScalars& us, int clip, float* p, const float* g, float* m, float* v,
                                long long n, float lr, float beta1, float beta2, float eps, int* status,
                                int* refused, const float* dp_flag, float gscale, float* loss, void* stream,
                                const ShadowSegs* sh = nullptr, const ClipArgs* cl = nullptr) {
  DL4SS_REQUIRE(p && g && m && v && n >= 0);
  if (n == 0) return 0;
  const unsigned grid = (unsigned)min(8192LL, (n / 4 + 255) / 256 + 1);
  const bool shadows = sh && sh->n > 0;
#define UPD_LAUNCH(KIND_, CLIP_, SH_)                                                                                 \
  hipLaunchKernelGGL((update_kernel<KIND_, CLIP_, SH_>), dim3(grid), dim3(256), 0, as_stream(stream), p, g, m, v, n,  \
                     lr, beta1, beta2, eps, us.bc1, us.bc2s, status, refused, dp_flag, gscale, loss,                  \
                     shadows ? *sh : ShadowSegs{}, cl ? *cl : ClipArgs{}, us.a1, us.a2)
#define UPD_CLIP(KIND_, CLIP_)                                                  \
  do {                                                                          \
    if (shadows) UPD_LAUNCH(KIND_, CLIP_, true); else UPD_LAUNCH(KIND_, CLIP_, false); \
  } while (0)
  DL4SS_REQUIRE((us.kind == UPD_ADAM || us.kind == UPD_NADAM) && clip >= CLIP_NONE && clip <= CLIP_KERAS);
  switch (us.kind * 3 + clip) {
    case UPD_ADAM * 3 + CLIP_NONE: UPD_CLIP(UPD_ADAM, CLIP_NONE); break;
    case UPD_ADAM * 3 + CLIP_TORCH: UPD_CLIP(UPD_ADAM, CLIP_TORCH); break;
#ifdef DL4SS_UPDATE_ALL  // optim.hip: every form; small.hip: Adam, unclipped or with torch's clip
    case UPD_ADAM * 3 + CLIP_KERAS: UPD_CLIP(UPD_ADAM, CLIP_KERAS); break;
    case UPD_NADAM * 3 + CLIP_NONE: UPD_CLIP(UPD_NADAM, CLIP_NONE); break;
    case UPD_NADAM * 3 + CLIP_TORCH: UPD_CLIP(UPD_NADAM, CLIP_TORCH); break;
    case UPD_NADAM * 3 + CLIP_KERAS: UPD_CLIP(UPD_NADAM, CLIP_KERAS); break;
#endif
    default: return (int)hipErrorInvalidValue;
  }
#undef UPD_CLIP
#undef UPD_LAUNCH
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// the shadow-segment arrays of the entry points, checked and packed for the kernel
static inline int shadow_segs(ShadowSegs& sh, long long n, int nseg, const long long* seg_off, const int* seg_rows,
                              const int* seg_cols, void* const* seg_y, const long long* seg_ldy) {
  DL4SS_REQUIRE(nseg >= 0 && nseg <= SHADOW_MAX && (nseg == 0 || (seg_off && seg_rows && seg_cols && seg_y && seg_ldy)));
  sh.n = nseg;
  for (int i = 0; i < nseg; ++i) {
    DL4SS_REQUIRE(seg_y[i] && seg_rows[i] >= 0 && seg_cols[i] > 0 && seg_ldy[i] >= seg_cols[i] && seg_off[i] >= 0 &&
                  seg_off[i] + (long long)seg_rows[i] * seg_cols[i] <= n && (long long)seg_rows[i] * seg_cols[i] < (1LL << 31));
    DL4SS_REQUIRE(((uintptr_t)seg_y[i] & 7) == 0);  // the 8-B quad stores
    sh.off[i] = seg_off[i];
    sh.len[i] = (long long)seg_rows[i] * seg_cols[i];
    sh.cols[i] = seg_cols[i];
    sh.ldy[i] = seg_ldy[i];
    sh.y[i] = reinterpret_cast<unsigned short*>(seg_y[i]);
  }
  return 0;
}

}  // namespace
