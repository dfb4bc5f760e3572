// What the fused attention + loss kernels share (attn_loss.hip: attn_kernel, attn_q4_kernel; attn_align.hip:
// align_kernel): the tiling of an utterance's rows over blocks, the row losses, the block reduction of the costs
// and the tile I/O.  Every helper keeps the expressions, operand order and accumulation order the kernels had
// when each wrote them out itself: the COST and the GRAD pass of a PIT step, and the kernel forms of one pass,
// must sum alike, bit for bit.
#pragma once
#include "common.h"

namespace attn_tile {

constexpr int NT = 256;    // lanes per block
constexpr int TILE = 256;  // rows per tile
// 4 tiles per block: with attn_q4_kernel at C2 -- 32 x 32 blocks, one round at 4 resident per CU --
// GRAD 65.8 / 66.7 / 71.1 us at 4 / 2 / 3 tiles, COST + PIT select 25.2 / 25.8 / 27.1 us
// (profiles/r03_attn_q4.jsonl; round 2's attn_kernel preferred 3)
constexpr int TPB = 4;

// blocks per utterance of `rows` rows
inline int nblk(long long rows) {
  const long long n = (rows + TPB * TILE - 1) / (TPB * TILE);
  return n < 1 ? 1 : (int)n;
}

template <int K>
struct Perms;
template <>
struct Perms<1> { static constexpr int N = 1; static constexpr int P[1][1] = {{0}}; };
template <>
struct Perms<2> { static constexpr int N = 2; static constexpr int P[2][2] = {{0, 1}, {1, 0}}; };
template <>
struct Perms<3> {
  static constexpr int N = 6;
  static constexpr int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
};

// rows [rbeg, rend) of the utterance that block blockIdx.x of its nblk walks
struct RowRange { int rbeg, rend; };
__device__ __forceinline__ RowRange block_rows(int rows, int nblk) {
  const int per = (rows + nblk - 1) / nblk;
  const int rbeg = blockIdx.x * per;
  return {rbeg, min(rows, rbeg + per)};
}

// target index per channel of utterance b; perm null = identity
template <int K>
__device__ __forceinline__ void load_perm(const int* perm, int b, int (&pm)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) pm[k] = perm ? perm[b * K + k] : k;
}

// ---- the magnitude row loss's gradient (EvalVer.py:641,659-666): dL/dlogit_k from the masks m, the magnitude x,
// channel k's target yp (the caller's select over its K targets by the permutation: through a reference the select
// keeps the targets in memory at K = 3) and ds = sum_k m_k - 1; a: the kernel's arguments (s1, s2).  ADV: ge is the row's
// second gradient at the prediction m_k x (the adversarial step).  (The costs themselves, and the cRM row, stay
// written out in each kernel: DESIGN.md, "Attention kernels: one template per body".)
template <bool ADV, int K, class Args>
__device__ __forceinline__ float mag_dl(const Args& a, int k, const float (&m)[K], float x, float yp, float ds,
                                        float ge) {
  const float g = 2.f * a.s1 * (m[k] * x - yp);
  const float dm = ADV ? (g + ge) * x + 2.f * a.s2 * ds : g * x + 2.f * a.s2 * ds;
  return dm * m[k] * (1.f - m[k]);
}

// ---- the block's costs into its part_loss record pl[NC], fixed order: the wave's lanes that count (all, or one
// per row where several lanes share a row) by wave_sum, then waves 0..3
template <int NC>
__device__ __forceinline__ void reduce_costs(const float (&cost)[NC], bool counts, float* pl) {
  __shared__ float sred[NT / 64][NC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const float s = wave_sum(counts ? cost[i] : 0.f);
    if (lane == 0) sred[wave][i] = s;
  }
  __syncthreads();
  if (tid < NC) pl[tid] = sred[0][tid] + sred[1][tid] + sred[2][tid] + sred[3][tid];
}

// ---- n fp32 values between a tile in LDS and global memory, coalesced, either way.  vec: the caller's test
// that 16-B accesses are aligned on the global side (the LDS tile is)
__device__ __forceinline__ void copy_f32(float* dst, const float* src, int n, bool vec) {
  const int tid = threadIdx.x;
  if (vec) {
    const int n4 = n >> 2;
    for (int i = tid; i < n4; i += NT) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    for (int i = (n4 << 2) + tid; i < n; i += NT) dst[i] = src[i];
  } else {
    for (int i = tid; i < n; i += NT) dst[i] = src[i];
  }
}

// ---- the tile's bf16 dPre (rows r0 .. r0 + nr of utterance b, EP 4-B words = pairs of values each) into rows
// (b T + t) of the (B T, ldpb) matrix the Linear's backward GEMMs read.  Row (t, f) lives at t ldpb + f 2 EP, so
// the tile is one contiguous run per frame it touches (at most 3 at F = 129); the columns >= F 2 EP of a row are
// never written.  Each run goes out as 16-B stores from its first 16-B aligned destination word on, with its
// <= 3 head and <= 3 tail words stored singly: a quarter of the store instructions of a word-per-lane copy.
// word(i): the tile's i-th word (the source need not be 16-B aligned)
template <int EP, class Word>
__device__ __forceinline__ void store_dpre_bf16(unsigned* dPreB, long long ldpb, int b, int T, int F, int r0, int nr,
                                                Word word) {
  const int tid = threadIdx.x;
  const long long rowb = (long long)b * T;
  const int ntot = nr * EP;
  for (int t = r0 / F, sw = 0; sw < ntot; ++t) {
    const int ew = min(ntot, ((t + 1) * F - r0) * EP);  // end of frame t's words in the tile
    unsigned* dst = dPreB + ((rowb + t) * ldpb >> 1) + (long long)(r0 - t * F) * EP;  // + word of the tile
    const int lead = (int)((4 - (((uintptr_t)(dst + sw)) >> 2)) & 3);  // words before the first aligned one
    const int i0 = min(ew, sw + lead);
    const int nq = (ew - i0) >> 2;
    for (int q = tid; q < nq; q += NT) {
      const int i = i0 + 4 * q;
      *reinterpret_cast<uint4*>(dst + i) = make_uint4(word(i), word(i + 1), word(i + 2), word(i + 3));
    }
    const int te = i0 + 4 * nq;  // tail words [te, ew), head words [sw, i0)
    if (tid < i0 - sw) dst[sw + tid] = word(sw + tid);
    if (tid >= 4 && tid - 4 < ew - te) dst[te + tid - 4] = word(te + tid - 4);
    sw = ew;
  }
}

}  // namespace attn_tile
