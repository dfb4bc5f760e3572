// Fused speaker-query mask attention + separation loss + its backward.
//
// Replaces, for the magnitude path (TDAA_beta/main_run_sstune_EvalVer.py:615-666,
// Torch_multi/main_run.py:478-506):
//     V.expand(B,K,...).contiguous()          (414 MB copy at B=32)
//     baddbmm(V, q) -> sigmoid                 mask (B,K,T,F)
//     predict = mask * |X| ; MSE(predict, Y) + 0.5 * MSE(sum_k mask, 1)
// and for the cRM path (main_run_sstune_cRM_EvalVer.py:259-271, 688, 720-743):
//     Mc = 10 tanh(V.q_{re,im}); M = -1/0.1 log((10 - Mc)/(10 + Mc));
//     P = M (x) X (complex product); MSE(P_re, Y_re) + MSE(P_im, Y_im)
// together with the whole backward down to dPre = dL/d(h W^T + b) of the
// Linear+tanh that produced V, and dq = dL/dq.
//
// One pass reads each V row (E floats) exactly once: a workgroup stages a 256-row
// tile of V with coalesced 16-B loads into LDS, each lane owns one (b,t,f) row
// (8-B LDS reads: conflict-free for E = 50), computes the K logits / masks /
// costs, and in the GRAD pass writes the dPre row back into the same LDS tile
// for a coalesced store.  Loss terms and dq are reduced per workgroup (wave
// shuffles + LDS) into per-block partials that a finalize kernel sums in fixed
// order (bitwise deterministic).  PIT: the COST pass produces the K x K pairwise
// cost matrix per utterance, `pit_select` picks the lowest-index minimising
// permutation, the GRAD pass uses it; label order (the reference) = identity.
#include "common.h"
#include <hip/hip_bf16.h>

namespace {

constexpr int NT = 256;
constexpr int TILE = 256;  // rows per tile

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

struct AttnArgs {
  int B, T, F, rows_per_b, nblk;  // rows_per_b = T*F ; nblk = blocks per utterance
  const float* V;                 // (B, T*F, E)
  const unsigned short* Vb;       // the same as bf16 (the fast path's Linear writes V in bf16); V unused then
  const float* q;                 // (B, K, QW)
  const float* X;                 // mag: (b*xs + row) ; cRM: (b*xs + row)*2
  long long xs;
  const float* Y;                 // target k of b: Y + b*ys + k*yks (+row, cRM *2)
  long long ys, yks;
  const int* perm;                // (B, K) target index per channel, null = identity
  float s1, s2;                   // loss scales: MSE term, sum-to-one term
  float* dPre;                    // (B, T*F, E) GRAD pass output (fp32; null when dPreB is given)
  unsigned* dPreB;                // GRAD pass bf16 output: row (b*T + t) of F*E values at stride ldpb (bf16)
  long long ldpb;
  float* part_loss;               // (B, nblk, K*K + 1)
  float* part_dq;                 // (B, nblk, K, QW)
  float* mask_out;                // optional (B, K, T*F) [cRM: x2]
  float* pred_out;                // optional (B, K, T*F) [cRM: x2]
};

// ADV (the adversarial step): the GRAD pass adds a second gradient at the prediction pred = mask |X|,
// gext (B, K, T*F) in pred_out's layout (the Discriminator's conv1 dX): dm = (2 s1 (m x - y) + gext) x +
// 2 s2 ds.  A compile-time form: the kernels without it are the same code as before.
template <int E, int K, bool CRM, bool GRAD, bool VB>
__global__ __launch_bounds__(NT) void attn_kernel(AttnArgs a) {
  constexpr bool ADV = false;
  const float* const gext = nullptr;
#include "attn_kernel_body.h"
}

template <int E, int K, bool VB>
__global__ __launch_bounds__(NT) void attn_adv_kernel(AttnArgs a, const float* __restrict__ gext) {
  constexpr bool CRM = false, GRAD = true, ADV = true;
#include "attn_kernel_body.h"
}

// The bf16-V magnitude path (the throughput step), one QUAD of lanes per (b,t,f) row.
// attn_kernel gives each lane a whole row (E = 50 values: 100 logit FMAs, 100 dPre FMAs and a
// 256-long serial dq chain per tile on 100 lanes: latency-bound at ~2.5 TB/s); a lane holding
// all K*E dq sums in registers (221 VGPRs, 2 waves per SIMD) was slower still.  Here lane j of a
// quad owns the row's bf16 pairs w = j, j+4, j+8, ... (7 of the 25 at E = 50), so a lane keeps
// only its 14 q values and 14 dq sums per query in registers (~4 waves per SIMD): partial logits
// over its pairs, the quad's sum by two DPP quad permutes (bitwise the same value in all four
// lanes), then dl, the lane's dPre pairs (written back as bf16 over its own V words) and its dq
// terms.  V reaches LDS by LDS-DMA (`global_load_lds_dwordx4`, no staging registers) from the 16-B
// aligned word below the tile (the tile's first word sits `off` words into the LDS image); dPre leaves by coalesced 4-B stores whose
// (t, f) destination changes only at frame boundaries, as 16-B stores from each frame segment's first
// 16-B aligned destination word.  Only the
// logits' summation order differs from attn_kernel (quad partials instead of one serial chain);
// dq is per-lane partials -> wave xor-shuffle tree -> waves 0..3 in order (deterministic).
__device__ __forceinline__ float quad_xor1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));  // [1,0,3,2]
}
__device__ __forceinline__ float quad_xor2(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));  // [2,3,0,1]
}

typedef __attribute__((address_space(3))) void attn_lds_void;
__device__ __attribute__((aligned(16))) const unsigned g_attn_zero[4] = {0u, 0u, 0u, 0u};

// VF (round 5): fp32 V (the split-precision "bf16s" steps keep V = tanh(Linear) in fp32): the tile
// arrives as fp32 words (a pair = 8 B, read as one float2), the bf16 dPre pairs go to a separate LDS
// image (sdp) for the same copy-out; everything else -- the quad's arithmetic and summation order,
// the bf16 dPre, dq -- as in the bf16-V form.  The generic attn_kernel ran this step at ~2 TB/s
// (C4 bf16s: 156 us per step for its one GRAD launch).
template <int E, int K, bool GRAD, bool VF = false, bool CRM = false>
__global__ __launch_bounds__(NT, (K == 3 && GRAD) || VF || CRM ? 2 : 4) void attn_q4_kernel(AttnArgs a) {
  static_assert(E % 2 == 0, "bf16 pairs");
  constexpr bool ADV = false;
  const float* const gext = nullptr;
#include "attn_q4_body.h"
}

// the adversarial GRAD pass on the quad layout: bf16 V (VF false) or fp32 V with bf16 dPre (VF true).
// K = 2 on bf16 V: the RPQ x K prefetched gext values do not fit the 128 VGPRs of 4 workgroups per CU
// (28 B of scratch per lane); at 3 per CU (168 VGPRs) nothing spills
template <int E, int K, bool VF>
__global__ __launch_bounds__(NT, K == 3 || VF ? 2 : K == 2 ? 3 : 4) void attn_q4_adv_kernel(
    AttnArgs a, const float* __restrict__ gext) {
  static_assert(E % 2 == 0, "bf16 pairs");
  constexpr bool GRAD = true, CRM = false, ADV = true;
#include "attn_q4_body.h"
}

// PIT selection: per utterance, lowest-index permutation minimising sum_k C[k][perm k].  One
// wave per utterance: lane l sums the block partials l, l + 64, ... in order, then a fixed
// butterfly tree over the lanes (deterministic; one thread walking all nblk partials serially
// took ~12 us at C2)
template <int K>
__global__ __launch_bounds__(64) void pit_select_kernel(const float* __restrict__ part, int B, int nblk,
                                                        int* __restrict__ perm) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float C[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) C[i] = 0.f;
  for (int blk = lane; blk < nblk; blk += 64)
#pragma unroll
    for (int i = 0; i < K * K; ++i) C[i] += part[((long long)b * nblk + blk) * (K * K + 1) + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < K * K; ++i) C[i] += __shfl_xor(C[i], off);
  if (lane != 0) return;
  int best = 0;
  float bc = 0.f;
  for (int p = 0; p < Perms<K>::N; ++p) {
    float c = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) c += C[k * K + Perms<K>::P[p][k]];
    if (p == 0 || c < bc) { bc = c; best = p; }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) perm[b * K + k] = Perms<K>::P[best][k];
}

constexpr int FIN_CH = 8;      // finalize: loss items per thread loaded together
constexpr int FIN_PMAX = 1024;  // finalize: permutation entries staged in LDS (B K <= this; else direct loads)
// loss = s1 * sum_b sum_k C[b][k][perm k] + s2 * S ; also dq = sum_blk part_dq (fixed order)
template <int K>
__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ part, int B, int nblk,
                                                       const int* __restrict__ perm, float s1, float s2,
                                                       float* __restrict__ loss_out,
                                                       const float* __restrict__ part_dq, int qw,
                                                       float* __restrict__ dq) {
  // block 0: loss, 256 fixed-stride fp64 partial sums + fixed-order tree (deterministic)
  if (blockIdx.x == 0) {
    __shared__ double r1[256], r2[256];
    __shared__ int sperm[FIN_PMAX];
    double l1 = 0.0, l2 = 0.0;
    // the permutations staged in LDS first, then each thread's items loaded in chunks of FIN_CH
    // before they are summed in item order (round 6: a perm load then the cost loads per item was
    // two dependent rounds per item)
    const bool lp = perm && B * K <= FIN_PMAX;
    if (lp)
      for (int i = threadIdx.x; i < B * K; i += 256) sperm[i] = perm[i];
    __syncthreads();
    for (int i0 = threadIdx.x; i0 < B * nblk; i0 += 256 * FIN_CH) {
      float c[FIN_CH][K + 1];
#pragma unroll
      for (int u = 0; u < FIN_CH; ++u) {
        const int i = min(i0 + 256 * u, B * nblk - 1), b = i / nblk;
        const float* p = part + (long long)i * (K * K + 1);
#pragma unroll
        for (int k = 0; k < K; ++k)
          c[u][k] = p[k * K + (perm ? (lp ? sperm[b * K + k] : perm[b * K + k]) : k)];
        c[u][K] = p[K * K];
      }
#pragma unroll
      for (int u = 0; u < FIN_CH; ++u) {
        if (i0 + 256 * u < B * nblk) {
#pragma unroll
          for (int k = 0; k < K; ++k) l1 += c[u][k];
          l2 += c[u][K];
        }
      }
    }
    r1[threadIdx.x] = l1;
    r2[threadIdx.x] = l2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) {
        r1[threadIdx.x] += r1[threadIdx.x + w];
        r2[threadIdx.x] += r2[threadIdx.x + w];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      loss_out[0] = (float)(s1 * r1[0] + s2 * r2[0]);
      loss_out[1] = (float)(s1 * r1[0]);
      loss_out[2] = (float)(s2 * r2[0]);
    }
    return;
  }
  // blocks 1..: dq = sum over the utterance's blocks, fixed order
  if (dq) {
    const int n = B * K * qw;
    for (int i = (blockIdx.x - 1) * blockDim.x + threadIdx.x; i < n; i += (gridDim.x - 1) * blockDim.x) {
      const int b = i / (K * qw), j = i % (K * qw);
      const float* pd = part_dq + (long long)b * nblk * K * qw + j;
      float a0 = 0.f, a1 = 0.f;
      // even blocks into a0, odd into a1, in block order; the loads of 32 blocks issued together
      for (int b0 = 0; b0 < nblk; b0 += 32) {
        float x[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) x[u] = pd[(long long)min(b0 + u, nblk - 1) * K * qw];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          const bool in = b0 + u < nblk;
          a0 = (in && !(u & 1)) ? a0 + x[u] : a0;
          a1 = (in && (u & 1)) ? a1 + x[u] : a1;
        }
      }
      dq[i] = a0 + a1;
    }
  }
}

template <int E, int K, bool CRM, bool VB>
int launch_attn(bool grad, const AttnArgs& a, hipStream_t st) {
  dim3 grid(a.nblk, a.B);
  if constexpr (!(CRM && K == 3)) {  // the throughput steps' path (16-B aligned V; bf16 dPre), magnitude and
                                     // cRM (K = 3 cRM: the quad kernel's 2 x 3 query halves spill; attn_kernel)
    // fp32 V or cRM: only for a bf16-dPre caller (which passes dPre_bf16 to its COST pass too, so both
    // passes of a PIT step sum the logits alike); the fp32 parity step keeps attn_kernel
    const bool q4 = (VB && !CRM) ? (a.dPreB || !grad) : a.dPreB != nullptr;
    if (q4 && ((uintptr_t)(VB ? (const void*)a.Vb : (const void*)a.V) & 15) == 0) {
      if (grad)
        hipLaunchKernelGGL((attn_q4_kernel<E, K, true, !VB, CRM>), grid, dim3(NT), 0, st, a);
      else
        hipLaunchKernelGGL((attn_q4_kernel<E, K, false, !VB, CRM>), grid, dim3(NT), 0, st, a);
      DL4SS_CHECK_LAUNCH();
      return 0;
    }
  }
  if (grad)
    hipLaunchKernelGGL((attn_kernel<E, K, CRM, true, VB>), grid, dim3(NT), 0, st, a);
  else
    hipLaunchKernelGGL((attn_kernel<E, K, CRM, false, VB>), grid, dim3(NT), 0, st, a);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// the adversarial GRAD pass: the kernel form launch_attn picks for the same arguments, with gext
template <int E, int K, bool VB>
int launch_attn_adv(const AttnArgs& a, const float* gext, hipStream_t st) {
  dim3 grid(a.nblk, a.B);
  if (a.dPreB && ((uintptr_t)(VB ? (const void*)a.Vb : (const void*)a.V) & 15) == 0)
    hipLaunchKernelGGL((attn_q4_adv_kernel<E, K, !VB>), grid, dim3(NT), 0, st, a, gext);
  else
    hipLaunchKernelGGL((attn_adv_kernel<E, K, VB>), grid, dim3(NT), 0, st, a, gext);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

template <bool VB>
int dispatch_adv(int E, int K, const AttnArgs& a, const float* gext, hipStream_t st) {
  if (E != 50) return (int)hipErrorInvalidValue;
  if (K == 1) return launch_attn_adv<50, 1, VB>(a, gext, st);
  if (K == 2) return launch_attn_adv<50, 2, VB>(a, gext, st);
  if (K == 3) return launch_attn_adv<50, 3, VB>(a, gext, st);
  return (int)hipErrorInvalidValue;
}

template <bool VB>
int dispatch_v(int E, int K, int crm, bool grad, const AttnArgs& a, hipStream_t st) {
  if (E != 50) return (int)hipErrorInvalidValue;
  if (!crm) {
    if (K == 1) return launch_attn<50, 1, false, VB>(grad, a, st);
    if (K == 2) return launch_attn<50, 2, false, VB>(grad, a, st);
    if (K == 3) return launch_attn<50, 3, false, VB>(grad, a, st);
  } else {
    if (K == 1) return launch_attn<50, 1, true, VB>(grad, a, st);
    if (K == 2) return launch_attn<50, 2, true, VB>(grad, a, st);
    if (K == 3) return launch_attn<50, 3, true, VB>(grad, a, st);
  }
  return (int)hipErrorInvalidValue;
}

int attn_common(int pass, int crm, int B, int K, int T, int F, int E, const float* V, const void* Vb, const float* q,
                const float* X, long long x_bstride, const float* Y, long long y_bstride, long long y_kstride,
                const int* perm, float s1, float s2, float* dPre, void* dPre_bf16, long long dpre_bf16_ld,
                float* part_loss, float* part_dq, float* mask_out, float* pred_out, void* stream,
                const float* gext = nullptr) {
  DL4SS_REQUIRE(B > 0 && K >= 1 && K <= 3 && T > 0 && F > 0 && q && X && Y && part_loss);
  DL4SS_REQUIRE(pass == 0 || ((dPre || dPre_bf16) && part_dq));
  DL4SS_REQUIRE(!dPre_bf16 || (E % 2 == 0 && dpre_bf16_ld % 2 == 0 && dpre_bf16_ld >= (long long)F * E &&
                               ((uintptr_t)dPre_bf16 & 3) == 0));
  AttnArgs a{};
  a.B = B; a.T = T; a.F = F; a.rows_per_b = T * F; a.nblk = dl4ss_attn_nblk(T, F);
  a.V = V; a.Vb = reinterpret_cast<const unsigned short*>(Vb);
  a.q = q; a.X = X; a.xs = x_bstride; a.Y = Y; a.ys = y_bstride; a.yks = y_kstride;
  a.perm = perm; a.s1 = s1; a.s2 = s2; a.dPre = dPre; a.part_loss = part_loss; a.part_dq = part_dq;
  a.dPreB = reinterpret_cast<unsigned*>(dPre_bf16); a.ldpb = dpre_bf16_ld;
  a.mask_out = mask_out; a.pred_out = pred_out;
  if (gext)
    return Vb ? dispatch_adv<true>(E, K, a, gext, as_stream(stream))
              : dispatch_adv<false>(E, K, a, gext, as_stream(stream));
  return Vb ? dispatch_v<true>(E, K, crm, pass == 1, a, as_stream(stream))
            : dispatch_v<false>(E, K, crm, pass == 1, a, as_stream(stream));
}
}  // namespace

DL4SS_API int dl4ss_attn_nblk(int T, int F) {
  // 4 tiles per block: with attn_q4_kernel at C2 -- 32 x 32 blocks, one round at 4 resident per CU --
  // GRAD 65.8 / 66.7 / 71.1 us at 4 / 2 / 3 tiles, COST + PIT select 25.2 / 25.8 / 27.1 us
  // (profiles/r03_attn_q4.jsonl; round 2's attn_kernel preferred 3)
  constexpr int tpb = 4;
  const int rows = T * F;
  int nblk = (rows + tpb * TILE - 1) / (tpb * TILE);
  return nblk < 1 ? 1 : nblk;
}

// pass: 0 = COST (costs / masks only), 1 = GRAD (costs + dPre + dq partials)
DL4SS_API int dl4ss_mask_attn_loss(int pass, int crm, int B, int K, int T, int F, int E, const float* V,
                                   const float* q, const float* X, long long x_bstride, const float* Y,
                                   long long y_bstride, long long y_kstride, const int* perm, float s1, float s2,
                                   float* dPre, float* part_loss, float* part_dq, float* mask_out,
                                   float* pred_out, void* stream) {
  DL4SS_REQUIRE(pass == 0 || dPre);
  return dl4ss_mask_attn_loss_ex(pass, crm, B, K, T, F, E, V, q, X, x_bstride, Y, y_bstride, y_kstride, perm, s1, s2,
                                 dPre, nullptr, 0, part_loss, part_dq, mask_out, pred_out, stream);
}

DL4SS_API int dl4ss_mask_attn_loss_ex(int pass, int crm, int B, int K, int T, int F, int E, const float* V,
                                      const float* q, const float* X, long long x_bstride, const float* Y,
                                      long long y_bstride, long long y_kstride, const int* perm, float s1, float s2,
                                      float* dPre, void* dPre_bf16, long long dpre_bf16_ld, float* part_loss,
                                      float* part_dq, float* mask_out, float* pred_out, void* stream) {
  DL4SS_REQUIRE(V);
  return attn_common(pass, crm, B, K, T, F, E, V, nullptr, q, X, x_bstride, Y, y_bstride, y_kstride, perm, s1, s2,
                     dPre, dPre_bf16, dpre_bf16_ld, part_loss, part_dq, mask_out, pred_out, stream);
}

DL4SS_API int dl4ss_mask_attn_loss_bf16v(int pass, int crm, int B, int K, int T, int F, int E, const void* V_bf16,
                                         const float* q, const float* X, long long x_bstride, const float* Y,
                                         long long y_bstride, long long y_kstride, const int* perm, float s1,
                                         float s2, float* dPre, void* dPre_bf16, long long dpre_bf16_ld,
                                         float* part_loss, float* part_dq, float* mask_out, float* pred_out,
                                         void* stream) {
  DL4SS_REQUIRE(V_bf16 && ((uintptr_t)V_bf16 & 3) == 0 && E % 2 == 0);
  return attn_common(pass, crm, B, K, T, F, E, nullptr, V_bf16, q, X, x_bstride, Y, y_bstride, y_kstride, perm, s1,
                     s2, dPre, dPre_bf16, dpre_bf16_ld, part_loss, part_dq, mask_out, pred_out, stream);
}

// The GRAD pass of the magnitude path with a second gradient at the prediction pred = mask |X|:
// dpred_extra (B, K, T*F) fp32 in pred_out's layout (the adversarial step: the Discriminator's input
// gradient on the predicted maps).  Everything else as dl4ss_mask_attn_loss_ex's pass 1 (crm 0): the loss
// partials are those of the call without it, bit for bit.
DL4SS_API int dl4ss_mask_attn_loss_adv(int B, int K, int T, int F, int E, const float* V, const float* q,
                                       const float* X, long long x_bstride, const float* Y, long long y_bstride,
                                       long long y_kstride, const int* perm, float s1, float s2,
                                       const float* dpred_extra, float* dPre, void* dPre_bf16,
                                       long long dpre_bf16_ld, float* part_loss, float* part_dq, float* mask_out,
                                       float* pred_out, void* stream) {
  DL4SS_REQUIRE(V && dpred_extra);
  return attn_common(1, 0, B, K, T, F, E, V, nullptr, q, X, x_bstride, Y, y_bstride, y_kstride, perm, s1, s2, dPre,
                     dPre_bf16, dpre_bf16_ld, part_loss, part_dq, mask_out, pred_out, stream, dpred_extra);
}

DL4SS_API int dl4ss_mask_attn_loss_adv_bf16v(int B, int K, int T, int F, int E, const void* V_bf16, const float* q,
                                             const float* X, long long x_bstride, const float* Y,
                                             long long y_bstride, long long y_kstride, const int* perm, float s1,
                                             float s2, const float* dpred_extra, float* dPre, void* dPre_bf16,
                                             long long dpre_bf16_ld, float* part_loss, float* part_dq,
                                             float* mask_out, float* pred_out, void* stream) {
  DL4SS_REQUIRE(V_bf16 && ((uintptr_t)V_bf16 & 3) == 0 && E % 2 == 0 && dpred_extra);
  return attn_common(1, 0, B, K, T, F, E, nullptr, V_bf16, q, X, x_bstride, Y, y_bstride, y_kstride, perm, s1, s2,
                     dPre, dPre_bf16, dpre_bf16_ld, part_loss, part_dq, mask_out, pred_out, stream, dpred_extra);
}

DL4SS_API int dl4ss_pit_select(const float* part_loss, int B, int K, int nblk, int* perm, void* stream) {
  DL4SS_REQUIRE(part_loss && perm && B > 0 && K >= 1 && K <= 3);
  hipStream_t st = as_stream(stream);
  dim3 grid(B), blk(64);
  if (K == 1) hipLaunchKernelGGL(pit_select_kernel<1>, grid, blk, 0, st, part_loss, B, nblk, perm);
  if (K == 2) hipLaunchKernelGGL(pit_select_kernel<2>, grid, blk, 0, st, part_loss, B, nblk, perm);
  if (K == 3) hipLaunchKernelGGL(pit_select_kernel<3>, grid, blk, 0, st, part_loss, B, nblk, perm);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// loss_out[0] = total loss, [1] = MSE term, [2] = weighted sum-to-one term; dq (B,K,qw) = sum of partials
DL4SS_API int dl4ss_loss_finalize(const float* part_loss, int B, int K, int nblk, const int* perm, float s1,
                                  float s2, float* loss_out, const float* part_dq, int qw, float* dq,
                                  void* stream) {
  DL4SS_REQUIRE(part_loss && loss_out && B > 0 && K >= 1 && K <= 3);
  hipStream_t st = as_stream(stream);
  dim3 grid(1 + (dq ? cdiv((long long)B * K * (qw > 0 ? qw : 1), 256) : 0)), blk(256);
  if (K == 1) hipLaunchKernelGGL(finalize_kernel<1>, grid, blk, 0, st, part_loss, B, nblk, perm, s1, s2, loss_out, part_dq, qw, dq);
  if (K == 2) hipLaunchKernelGGL(finalize_kernel<2>, grid, blk, 0, st, part_loss, B, nblk, perm, s1, s2, loss_out, part_dq, qw, dq);
  if (K == 3) hipLaunchKernelGGL(finalize_kernel<3>, grid, blk, 0, st, part_loss, B, nblk, perm, s1, s2, loss_out, part_dq, qw, dq);
  DL4SS_CHECK_LAUNCH();
  return 0;
}
