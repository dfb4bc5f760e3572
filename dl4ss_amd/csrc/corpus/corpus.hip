// Device-resident corpus (include/corpus/dl4ss_corpus.h; its own library, libdl4ss_corpus.so): the clips of a training set stay in one flat pool on the
// device, int16 or fp32; a step sends clip ids, shifts and gains and ONE launch gathers, normalises, rotates,
// pads, scales and sums them into the step's sources and mixtures.
//
// The arithmetic is mixing.hip's (source_stats_kernel + mix_kernel), bit for bit on the same samples: per clip 8
// partials {fp64 sum, min, max} combined in ascending order, mean = float(sum / len), peak = max(mx - mean,
// mean - mn); per element (x[(i + s) mod len] - mean) * (gain * inv_peak) with fp contraction off, the mixture the
// fp32 sum over the sources in ascending order.  What differs is where the samples come from (the clip's own
// 16-B aligned base instead of a zero-padded row, so the unrotated loads are vector loads whatever N is) and that
// the statistics are computed once per corpus, not every step.
#include "../common.h"

#include "../../../include/corpus/dl4ss_corpus.h"

namespace {

constexpr int NSPLIT = 8;
struct ClipPart {
  double sum;
  float mn, mx;
};
static_assert(sizeof(ClipPart) == 16, "16-B partials");

// int16 PCM: q / 32768 is exact in fp32
__device__ __forceinline__ float sample(const short* p) { return (float)p[0] * 0x1p-15f; }
__device__ __forceinline__ float sample(const float* p) { return p[0]; }
// 4 samples from an address aligned to 4 samples: one 8-B (int16) or 16-B (fp32) load
__device__ __forceinline__ float4 sample4(const short* p) {
  const short4 q = *reinterpret_cast<const short4*>(p);
  return make_float4((float)q.x * 0x1p-15f, (float)q.y * 0x1p-15f, (float)q.z * 0x1p-15f, (float)q.w * 0x1p-15f);
}
__device__ __forceinline__ float4 sample4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// grid (n_clips, NSPLIT): source_stats_kernel over clip blockIdx.x's own samples
template <typename T>
__global__ __launch_bounds__(256) void clip_stats_kernel(const T* __restrict__ pool,
                                                         const long long* __restrict__ offsets,
                                                         const int* __restrict__ lengths,
                                                         ClipPart* __restrict__ part) {
  const int c = blockIdx.x, p = blockIdx.y;
  const T* x = pool + offsets[c];
  const int N = max(lengths[c], 0);
  const int chunk = ((N + NSPLIT - 1) / NSPLIT + 3) & ~3;
  const int i0 = min(N, p * chunk), i1 = min(N, i0 + chunk);
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = i0 + threadIdx.x * 4; i < i1; i += 1024) {
    if (i + 3 < i1) {
      const float4 v = sample4(x + i);
      s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
      mn = fminf(fminf(mn, fminf(v.x, v.y)), fminf(v.z, v.w));
      mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    } else {
      for (int k = i; k < i1; ++k) {
        const float v = sample(x + k);
        s += v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
      }
    }
  }
  s = wave_sum_d(s);
  mx = wave_max(mx);
  mn = -wave_max(-mn);
  __shared__ double sd[4];
  __shared__ float smn[4], smx[4];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) { sd[w] = s; smn[w] = mn; smx[w] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    ClipPart r;
    r.sum = (sd[0] + sd[1]) + (sd[2] + sd[3]);
    r.mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    r.mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    part[(long long)c * NSPLIT + p] = r;
  }
}

// one thread per clip: the combine at the head of mix_kernel
__global__ __launch_bounds__(256) void clip_stats_combine_kernel(const ClipPart* __restrict__ part,
                                                                 const int* __restrict__ lengths, int n_clips,
                                                                 float2* __restrict__ stats) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_clips) return;
  const int len = max(lengths[c], 0);
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int p = 0; p < NSPLIT; ++p) {
    const ClipPart r = part[(long long)c * NSPLIT + p];
    s += r.sum;
    mn = fminf(mn, r.mn);
    mx = fmaxf(mx, r.mx);
  }
  const float meanf = len > 0 ? (float)(s / len) : 0.f;
  const float pk = len > 0 ? fmaxf(mx - meanf, meanf - mn) : 0.f;
  stats[c] = make_float2(meanf, pk > 0.f ? 1.0f / pk : 0.f);
}

// grid (ceil(N / 1024), B), 4 samples per thread: mix_kernel with each source read from its clip.  Sources
// K..Ks-1 are summed into the mixture only.  fp contraction off, as there.
template <typename T>
__global__ __launch_bounds__(256) void mix_corpus_kernel(const T* __restrict__ pool,
                                                         const long long* __restrict__ offsets,
                                                         const int* __restrict__ lengths,
                                                         const float2* __restrict__ stats, int n_clips,
                                                         const int* __restrict__ clips,
                                                         const int* __restrict__ shifts,
                                                         const float* __restrict__ gains, int K, int Ks, int N,
                                                         float* __restrict__ out_src, float* __restrict__ out_mix,
                                                         int* __restrict__ out_len, int* __restrict__ bad) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  __shared__ long long soff[16];
  __shared__ float2 sstat[16];
  __shared__ float sgain[16];
  __shared__ int slen[16], sshift[16];
  if (threadIdx.x < Ks) {
    const long long j = (long long)b * Ks + threadIdx.x;
    const int c = clips[j];
    long long off = 0;
    float2 st = make_float2(0.f, 0.f);
    int len = 0, sh = 0;
    if (c >= 0 && c < n_clips) {  // the tables are read through a valid id only
      off = offsets[c];
      len = min(max(lengths[c], 0), N);
      st = stats[c];
    } else if (blockIdx.x == 0) {
      atomicAdd(bad, 1);  // (an integer atomic: one count per silent source)
    }
    if (shifts && len > 0) {
      sh = shifts[j] % len;
      if (sh < 0) sh += len;
    }
    soff[threadIdx.x] = off;
    sstat[threadIdx.x] = st;
    sgain[threadIdx.x] = gains[j] * st.y;
    slen[threadIdx.x] = len;
    sshift[threadIdx.x] = sh;
    if (out_len && blockIdx.x == 0) out_len[j] = len;
  }
  __syncthreads();
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= N) return;
  const bool vec_out = (N & 3) == 0;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < Ks; ++k) {
    const T* x = pool + soff[k];
    const float mean = sstat[k].x, g = sgain[k];
    const int len = slen[k], sh = sshift[k];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);  // zero beyond the clip's own length
    if (sh == 0 && i + 3 < len) {  // the clip's base is 16-B aligned and i a multiple of 4
      v = sample4(x + i);
      v.x = (v.x - mean) * g; v.y = (v.y - mean) * g;
      v.z = (v.z - mean) * g; v.w = (v.w - mean) * g;
    } else {  // rotated: out[i] = x[(i + sh) mod len] for i < len; or the clip's last, partial quad
      float* a = &v.x;
      for (int q = 0; q < 4; ++q) {
        if (i + q < len) {
          int j = i + q + sh;
          j -= j >= len ? len : 0;
          a[q] = (sample(x + j) - mean) * g;
        }
      }
    }
    if (k < K) {
      float* o = out_src + ((long long)b * K + k) * N;
      if (vec_out) {
        *reinterpret_cast<float4*>(o + i) = v;
      } else {
        const float* a = &v.x;
        for (int q = 0; q < 4 && i + q < N; ++q) o[i + q] = a[q];
      }
    }
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  float* m = out_mix + (long long)b * N;
  if (vec_out) {
    *reinterpret_cast<float4*>(m + i) = acc;
  } else {
    const float* a = &acc.x;
    for (int q = 0; q < 4 && i + q < N; ++q) m[i + q] = a[q];
  }
}

inline bool known_dtype(int dtype) { return dtype == DL4SS_CORPUS_I16 || dtype == DL4SS_CORPUS_F32; }

}  // namespace

DL4SS_API int dl4ss_corpus_stats(const void* pool, int dtype, const long long* offsets, const int* lengths,
                                 int n_clips, float* ws, float* clip_stats, void* stream) {
  DL4SS_REQUIRE(known_dtype(dtype) && n_clips >= 0);
  if (n_clips == 0) return 0;
  DL4SS_REQUIRE(pool && offsets && lengths && ws && clip_stats);
  DL4SS_REQUIRE(((uintptr_t)pool & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)clip_stats & 7) == 0);
  ClipPart* part = reinterpret_cast<ClipPart*>(ws);
  if (dtype == DL4SS_CORPUS_I16)
    hipLaunchKernelGGL(clip_stats_kernel<short>, dim3(n_clips, NSPLIT), dim3(256), 0, as_stream(stream),
                       static_cast<const short*>(pool), offsets, lengths, part);
  else
    hipLaunchKernelGGL(clip_stats_kernel<float>, dim3(n_clips, NSPLIT), dim3(256), 0, as_stream(stream),
                       static_cast<const float*>(pool), offsets, lengths, part);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL(clip_stats_combine_kernel, dim3(cdiv(n_clips, 256)), dim3(256), 0, as_stream(stream), part,
                     lengths, n_clips, reinterpret_cast<float2*>(clip_stats));
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_mix_corpus(const void* pool, int dtype, const long long* offsets, const int* lengths,
                               const float* clip_stats, int n_clips, const int* clips, const int* shifts,
                               const float* gains, int B, int K, int Ks, int N, float* out_src, float* out_mix,
                               int* out_len, int* bad, void* stream) {
  DL4SS_REQUIRE(known_dtype(dtype) && n_clips >= 1);
  DL4SS_REQUIRE(B >= 0 && B <= 65535 && K >= 1 && K <= Ks && Ks <= 16 && N >= 1 && N <= (1 << 30));
  if (B == 0) return 0;  // empty batch: no-op (an empty tensor's pointer may be null)
  DL4SS_REQUIRE(pool && offsets && lengths && clip_stats && clips && gains && out_src && out_mix && bad);
  DL4SS_REQUIRE(((uintptr_t)pool & 15) == 0 && ((uintptr_t)clip_stats & 7) == 0);
  // (the vector stores' alignment: rows start at multiples of N floats)
  DL4SS_REQUIRE((N & 3) != 0 || ((((uintptr_t)out_src) | ((uintptr_t)out_mix)) & 15) == 0);
  const float2* st = reinterpret_cast<const float2*>(clip_stats);
  const dim3 grid(cdiv(N, 1024), B);
  if (dtype == DL4SS_CORPUS_I16)
    hipLaunchKernelGGL(mix_corpus_kernel<short>, grid, dim3(256), 0, as_stream(stream),
                       static_cast<const short*>(pool), offsets, lengths, st, n_clips, clips, shifts, gains, K, Ks, N,
                       out_src, out_mix, out_len, bad);
  else
    hipLaunchKernelGGL(mix_corpus_kernel<float>, grid, dim3(256), 0, as_stream(stream),
                       static_cast<const float*>(pool), offsets, lengths, st, n_clips, clips, shifts, gains, K, Ks, N,
                       out_src, out_mix, out_len, bad);
  DL4SS_CHECK_LAUNCH();
  return 0;
}
