// ATTENTION 'align' (additive attention) on the speaker-query mask:
//     mask = sigmoid(w3 . tanh(W1 V + W2 q))
// Cocktail/software/DL4SS_Keras/extend_layers.py:50-64 (the model the reference builds by default,
// nnet.py:88) and the 'align' branch of every Torch ATTENTION class
// (TDAA_beta/main_run_sstune_EvalVer.py:228-239: Linear_1 on the mixture embedding, Linear_2 on the
// query, tanh of their sum, Linear_3 to one logit, sigmoid).  E = A = 50 (align_hidden_size =
// hidden_size); the Linears have no bias.
//
//     U[b,r,:]   = W1 V[b,r,:]              p[b,k,:] = W2 q[b,k,:]
//     s[b,k,r,:] = tanh(U[b,r,:] + p[b,k,:])         logit = w3 . s       mask = sigmoid(logit)
// backward from dl = dL/dlogit:
//     dS = dl w3 (1 - s^2)    dU = sum_k dS    dV = dU W1    dW1 = sum_{b,r} dU (x) V
//     dp = sum_r dS           dq = dp W2       dW2 = sum_{b,k} dp (x) q      dw3 = sum dl s
//
// One kernel template serves the fused training step (COST / GRAD passes with the contract of
// dl4ss_mask_attn_loss_ex: same X / Y / perm / s1 / s2 / part_loss, so dl4ss_pit_select and
// dl4ss_loss_finalize take its partials unchanged) and the module-level forward / backward behind
// compat.myNet.ATTENTION.  A workgroup of 256 lanes walks 256-row tiles of one utterance:
//   1. the V tile is staged into LDS with coalesced 16-B loads (sv, 50 KB), one row per lane;
//   2. U = W1 v: the lane holds its row's 50 values in registers, W1 rows are wave-uniform
//      (scalar loads: the FMAs take them as scalar operands), U goes to the lane's row of a second
//      LDS tile (su, 50 KB);
//   3. s, the K logits, masks, costs and dl in registers (tanh as 1 - 2 / (exp(2x) + 1): absolute
//      error ~2e-7, which the logit's sum over 50 terms of |w3| <= 1/sqrt(50) keeps below 1e-7);
//   4. backward: dS_k (and dl s for dw3) are written to the su row one at a time and summed down the
//      tile's columns by lanes (a, r mod 5), then dU takes their place;
//   5. dW1 += dU^T V over the tile: 200 lanes own a 5 x 5 block of dW1 each, for the even or the odd
//      rows, reading dU and V of every row from the two LDS tiles (10 LDS words per 25 FMAs);
//   6. dV = dU W1 in registers (W1 rows uniform again), dPre = dV (1 - v^2) over the lane's sv row,
//      and the tile leaves with coalesced 16-B stores.
// All sums run in a fixed order; per-block partials (dW1 for even / odd rows, dp, dw3) are summed
// by dl4ss_attn_align_finalize in block order: no float atomics, bitwise reproducible.
// The two LDS tiles are 100 KB: one workgroup (one wave per SIMD) per CU.
// The bf16 step's forms (align_io_kernel, dl4ss_mask_attn_align_loss_ex) change the two ends only: step 1 reads
// bf16 V and widens it into the same fp32 sv, step 6 rounds dPre to bf16 on its way out, into rows of the GEMMs'
// pitch.  The kernel text is attn_align_body.h, included into both kernel definitions.
#include "common.h"
#include "../../include/dl4ss_align.h"

namespace {

constexpr int E = 50;            // embedding size = align hidden size
constexpr int NT = 256;
constexpr int TILE = 256;        // rows per tile
constexpr int TPB = 4;           // tiles per block
constexpr int NCH = 5;           // row classes of the column sums (250 lanes: 50 columns x 5)
constexpr int FIN_G = 16;        // finalize: groups of block records summed side by side
constexpr int W1P = 2 * E * E;   // dW1 partials of a block: even rows, odd rows

enum { COST = 0, GRAD = 1, MFWD = 2, MBWD = 3 };

// floats of one block's partial record: [dW1 even | dW1 odd | dp (K, E) | dw3 (E)]
__host__ __device__ constexpr int rec_floats(int K) { return W1P + K * E + E; }

struct AlignArgs {
  int B, R, nblk;          // R rows per utterance, nblk blocks per utterance
  const float* V;          // (B, R, E)
  const float* q;          // query k of b at q + b * qs + k * E
  long long qs;
  const float* X;          // fused: magnitude at b * xs + row
  long long xs;
  const float* Y;          // fused: target k of b at b * ys + k * yks + row
  long long ys, yks;
  const int* perm;         // (B, K) target per channel, null = identity
  float s1, s2;
  float* dPre;             // GRAD: (B, R, E), may be V itself; MBWD: dV, accumulated, may be null
  const float* dmask;      // MBWD: (B, R)
  float* part_loss;        // fused: (B, nblk, K*K + 1)
  float* part;             // backward: (B, nblk, rec_floats(K))
  float* mask_out;         // mask k of b at b * ms + k * R + row (optional in the fused passes)
  long long ms;
  float* pred_out;         // fused, optional: same layout
};

__device__ __forceinline__ float tanh_e(float x) {
  const float e = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// The bf16 step's I/O forms of the fused passes (align_io_kernel): V read as bf16, dPre written as bf16 rows
struct AlignIO {
  const unsigned short* Vb;  // VB: (B, R, E) bf16, 4-B aligned (the Linear's EPI_TANH_BF16 output)
  unsigned short* dPreB;     // DB: (B T, ldpb) bf16, 4-B aligned; row (t, f) of b at (b T + t) ldpb + f E
  long long ldpb;            // even, >= F E
  int T, F;                  // R = T F
};

template <int K, int MODE>
__global__ __launch_bounds__(NT) void align_kernel(AlignArgs a, const float* __restrict__ W1,
                                                    const float* __restrict__ W2, const float* __restrict__ w3) {
  constexpr bool VB = false, DB = false;
  constexpr AlignIO io{};
#include "attn_align_body.h"
}

// align_kernel with bf16 V (VB: a.V unused) and / or bf16 dPre at a row pitch (DB: a.dPre unused), compile-time
// forms of the same text: the arithmetic, the tiles and the order of every sum are align_kernel's, so the COST
// pass's partials on bf16 V equal, bit for bit, those on the same values in fp32
template <int K, int MODE, bool VB, bool DB>
__global__ __launch_bounds__(NT) void align_io_kernel(AlignArgs a, AlignIO io, const float* __restrict__ W1,
                                                       const float* __restrict__ W2, const float* __restrict__ w3) {
#include "attn_align_body.h"
}

// Finalize, stage 1: the dW1 (even + odd rows) and dw3 columns of the N block records, record groups
// g = 0 .. FIN_G - 1 side by side, each group's records in order.  grp (FIN_G, E*E + E).
__global__ __launch_bounds__(256) void align_fin_groups(const float* __restrict__ part, int N, int rec,
                                                        float* __restrict__ grp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E * E + E) return;
  const int g = blockIdx.y;
  const int per = (N + FIN_G - 1) / FIN_G;
  const int n0 = g * per, n1 = min(N, n0 + per);
  float acc = 0.f;
  if (i < E * E) {
    for (int n = n0; n < n1; ++n) {
      const float* p = part + (long long)n * rec;
      acc += p[i] + p[E * E + i];
    }
  } else {
    const int o = rec - E + (i - E * E);
    for (int n = n0; n < n1; ++n) acc += part[(long long)n * rec + o];
  }
  grp[g * (E * E + E) + i] = acc;
}

// Stage 2: dW1 / dw3 = the groups in order; dp[b][k][a] = the utterance's blocks in order.
__global__ __launch_bounds__(256) void align_fin_sum(const float* __restrict__ part, const float* __restrict__ grp,
                                                     int B, int K, int nblk, int rec, float* __restrict__ dW1,
                                                     float* __restrict__ dw3, float* __restrict__ dp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < E * E + E) {
    float acc = 0.f;
    for (int g = 0; g < FIN_G; ++g) acc += grp[g * (E * E + E) + i];
    if (i < E * E) dW1[i] = acc;
    else dw3[i - E * E] = acc;
    return;
  }
  const int j = i - (E * E + E);
  if (j >= B * K * E) return;
  const int b = j / (K * E), ka = j - b * (K * E);
  float acc = 0.f;
  for (int blk = 0; blk < nblk; ++blk) acc += part[((long long)b * nblk + blk) * rec + W1P + ka];
  dp[j] = acc;
}

// Stage 3: dq[b][k][:] = dp[b][k][:] W2 ; dW2 = sum_{b,k} dp[b][k] (x) q[b][k], (b, k) in order.
__global__ __launch_bounds__(256) void align_fin_dq(const float* __restrict__ dp, const float* __restrict__ q,
                                                    long long qs, const float* __restrict__ W2, int B, int K,
                                                    float* __restrict__ dq, long long dqs, float* __restrict__ dW2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < E * E) {
    const int aa = i / E, e = i - aa * E;
    float acc = 0.f;
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < K; ++k) acc = fmaf(dp[(b * K + k) * E + aa], q[(long long)b * qs + k * E + e], acc);
    dW2[i] = acc;
    return;
  }
  const int j = i - E * E;
  if (j >= B * K * E) return;
  const int bk = j / E, e = j - bk * E;
  const int b = bk / K, k = bk - b * K;
  float acc = 0.f;
  for (int aa = 0; aa < E; ++aa) acc = fmaf(dp[bk * E + aa], W2[aa * E + e], acc);
  dq[(long long)b * dqs + k * E + e] = acc;
}

int align_nblk(long long R) {
  const long long n = (R + TPB * TILE - 1) / (TPB * TILE);
  return n < 1 ? 1 : (int)n;
}

long long part_floats(int B, int K, int nblk) {
  return (long long)B * nblk * rec_floats(K) + (long long)FIN_G * (E * E + E) + (long long)B * K * E;
}

template <int MODE>
int launch_align(int K, const AlignArgs& a, const float* W1, const float* W2, const float* w3, hipStream_t st) {
  dim3 grid(a.nblk, a.B);
  if (K == 1) hipLaunchKernelGGL((align_kernel<1, MODE>), grid, dim3(NT), 0, st, a, W1, W2, w3);
  if constexpr (MODE == COST || MODE == GRAD) {
    if (K == 2) hipLaunchKernelGGL((align_kernel<2, MODE>), grid, dim3(NT), 0, st, a, W1, W2, w3);
    if (K == 3) hipLaunchKernelGGL((align_kernel<3, MODE>), grid, dim3(NT), 0, st, a, W1, W2, w3);
  }
  DL4SS_CHECK_LAUNCH();
  return 0;
}

template <int MODE, bool VB, bool DB>
int launch_align_io(int K, const AlignArgs& a, const AlignIO& io, const float* W1, const float* W2, const float* w3,
                    hipStream_t st) {
  dim3 grid(a.nblk, a.B);
  if (K == 1) hipLaunchKernelGGL((align_io_kernel<1, MODE, VB, DB>), grid, dim3(NT), 0, st, a, io, W1, W2, w3);
  if (K == 2) hipLaunchKernelGGL((align_io_kernel<2, MODE, VB, DB>), grid, dim3(NT), 0, st, a, io, W1, W2, w3);
  if (K == 3) hipLaunchKernelGGL((align_io_kernel<3, MODE, VB, DB>), grid, dim3(NT), 0, st, a, io, W1, W2, w3);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

int finalize(const float* part, int B, int K, int nblk, const float* q, long long qs, const float* W2, float* dq,
             long long dqs, float* dW1, float* dW2, float* dw3, hipStream_t st) {
  const int rec = rec_floats(K), N = B * nblk;
  float* grp = const_cast<float*>(part) + (long long)N * rec;
  float* dp = grp + FIN_G * (E * E + E);
  hipLaunchKernelGGL(align_fin_groups, dim3(cdiv(E * E + E, 256), FIN_G), dim3(256), 0, st, part, N, rec, grp);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL(align_fin_sum, dim3(cdiv(E * E + E + (long long)B * K * E, 256)), dim3(256), 0, st, part, grp, B,
                     K, nblk, rec, dW1, dw3, dp);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL(align_fin_dq, dim3(cdiv(E * E + (long long)B * K * E, 256)), dim3(256), 0, st, dp, q, qs, W2, B, K,
                     dq, dqs, dW2);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

DL4SS_API int dl4ss_attn_align_nblk(int R) { return R < 0 ? -1 : align_nblk(R); }

DL4SS_API long long dl4ss_attn_align_part_floats(int B, int K, int nblk) {
  if (B < 0 || K < 1 || K > 3 || nblk < 1) return -1;
  return part_floats(B, K, nblk);
}

DL4SS_API int dl4ss_attn_align_fwd(const float* V, const float* q, int q_stride, const float* W1, const float* W2,
                                   const float* w3, int Bq, int R, int E_, float* mask, long long mask_stride,
                                   void* stream) {
  DL4SS_REQUIRE(V && q && W1 && W2 && w3 && mask && Bq >= 0 && R >= 0 && E_ == E && q_stride >= E);
  DL4SS_REQUIRE(mask_stride >= R);
  if (Bq == 0 || R == 0) return 0;
  AlignArgs a{};
  a.B = Bq; a.R = R; a.nblk = align_nblk(R);
  a.V = V; a.q = q; a.qs = q_stride; a.mask_out = mask; a.ms = mask_stride;
  return launch_align<MFWD>(1, a, W1, W2, w3, as_stream(stream));
}

DL4SS_API int dl4ss_attn_align_bwd(const float* V, const float* q, int q_stride, const float* W1, const float* W2,
                                   const float* w3, const float* dmask, int Bq, int R, int E_, float* dV, float* part,
                                   long long part_floats_, float* dq, float* dW1, float* dW2, float* dw3,
                                   void* stream) {
  DL4SS_REQUIRE(V && q && W1 && W2 && w3 && dmask && part && dq && dW1 && dW2 && dw3);
  DL4SS_REQUIRE(Bq > 0 && R > 0 && E_ == E && q_stride >= E);
  const int nblk = align_nblk(R);
  DL4SS_REQUIRE(part_floats_ >= part_floats(Bq, 1, nblk));
  AlignArgs a{};
  a.B = Bq; a.R = R; a.nblk = nblk;
  a.V = V; a.q = q; a.qs = q_stride; a.dmask = dmask; a.dPre = dV; a.part = part;
  const int rc = launch_align<MBWD>(1, a, W1, W2, w3, as_stream(stream));
  if (rc) return rc;
  return finalize(part, Bq, 1, nblk, q, q_stride, W2, dq, E, dW1, dW2, dw3, as_stream(stream));
}

// pass: 0 = COST (costs / masks only), 1 = GRAD (costs + dPre + the partial records)
DL4SS_API int dl4ss_mask_attn_align_loss(int pass, int B, int K, int T, int F, int E_, const float* V, const float* q,
                                         const float* W1, const float* W2, const float* w3, const float* X,
                                         long long x_bstride, const float* Y, long long y_bstride,
                                         long long y_kstride, const int* perm, float s1, float s2, float* dPre,
                                         float* part_loss, float* part, long long part_floats_, float* mask_out,
                                         float* pred_out, void* stream) {
  DL4SS_REQUIRE(pass == 0 || pass == 1);
  DL4SS_REQUIRE(B > 0 && K >= 1 && K <= 3 && T > 0 && F > 0 && E_ == E);
  DL4SS_REQUIRE(V && q && W1 && W2 && w3 && X && Y && part_loss);
  const long long R = (long long)T * F;
  DL4SS_REQUIRE(R <= 0x7fffffff / E && x_bstride >= R && y_kstride >= R && y_bstride >= R);
  const int nblk = align_nblk(R);
  DL4SS_REQUIRE(pass == 0 || (dPre && part && part_floats_ >= part_floats(B, K, nblk)));
  AlignArgs a{};
  a.B = B; a.R = (int)R; a.nblk = nblk;
  a.V = V; a.q = q; a.qs = (long long)K * E;
  a.X = X; a.xs = x_bstride; a.Y = Y; a.ys = y_bstride; a.yks = y_kstride;
  a.perm = perm; a.s1 = s1; a.s2 = s2; a.dPre = dPre; a.part_loss = part_loss; a.part = part;
  a.mask_out = mask_out; a.ms = (long long)K * R; a.pred_out = pred_out;
  return pass == 1 ? launch_align<GRAD>(K, a, W1, W2, w3, as_stream(stream))
                   : launch_align<COST>(K, a, W1, W2, w3, as_stream(stream));
}

// dl4ss_mask_attn_align_loss with the bf16 step's I/O forms (include/dl4ss_align.h): V or V_bf16, dPre or
// dPre_bf16 at a row pitch.  Every refusal comes before any launch.
DL4SS_API int dl4ss_mask_attn_align_loss_ex(int pass, int B, int K, int T, int F, int E_, const float* V,
                                            const void* V_bf16, const float* q, const float* W1, const float* W2,
                                            const float* w3, const float* X, long long x_bstride, const float* Y,
                                            long long y_bstride, long long y_kstride, const int* perm, float s1,
                                            float s2, float* dPre, void* dPre_bf16, long long dpre_bf16_ld,
                                            float* part_loss, float* part, long long part_floats_, float* mask_out,
                                            float* pred_out, void* stream) {
  DL4SS_REQUIRE(pass == 0 || pass == 1);
  DL4SS_REQUIRE(B > 0 && K >= 1 && K <= 3 && T > 0 && F > 0 && E_ == E);
  DL4SS_REQUIRE((V != nullptr) != (V_bf16 != nullptr));
  DL4SS_REQUIRE(((uintptr_t)V_bf16 & 3) == 0);
  DL4SS_REQUIRE(q && W1 && W2 && w3 && X && Y && part_loss);
  const long long R = (long long)T * F;
  DL4SS_REQUIRE(R <= 0x7fffffff / E && x_bstride >= R && y_kstride >= R && y_bstride >= R);
  // (checked in the COST pass too, which is handed the GRAD pass's pointers and writes to neither)
  DL4SS_REQUIRE(!dPre_bf16 || (dpre_bf16_ld >= (long long)F * E && dpre_bf16_ld % 2 == 0 &&
                               ((uintptr_t)dPre_bf16 & 3) == 0));
  const int nblk = align_nblk(R);
  if (pass == 1) {
    DL4SS_REQUIRE((dPre != nullptr) != (dPre_bf16 != nullptr));
    DL4SS_REQUIRE(!(V_bf16 && dPre));  // bf16 V with fp32 dPre: no step forms it, not built
    DL4SS_REQUIRE(part && part_floats_ >= part_floats(B, K, nblk));
  }
  AlignArgs a{};
  a.B = B; a.R = (int)R; a.nblk = nblk;
  a.V = V; a.q = q; a.qs = (long long)K * E;
  a.X = X; a.xs = x_bstride; a.Y = Y; a.ys = y_bstride; a.yks = y_kstride;
  a.perm = perm; a.s1 = s1; a.s2 = s2; a.dPre = pass == 1 ? dPre : nullptr; a.part_loss = part_loss; a.part = part;
  a.mask_out = mask_out; a.ms = (long long)K * R; a.pred_out = pred_out;
  AlignIO io{};
  io.Vb = static_cast<const unsigned short*>(V_bf16);
  io.dPreB = static_cast<unsigned short*>(dPre_bf16); io.ldpb = dpre_bf16_ld; io.T = T; io.F = F;
  hipStream_t st = as_stream(stream);
  if (pass == 0)
    return V_bf16 ? launch_align_io<COST, true, false>(K, a, io, W1, W2, w3, st)
                  : launch_align<COST>(K, a, W1, W2, w3, st);
  if (dPre) return launch_align<GRAD>(K, a, W1, W2, w3, st);  // fp32 V, fp32 dPre: dl4ss_mask_attn_align_loss
  return V_bf16 ? launch_align_io<GRAD, true, true>(K, a, io, W1, W2, w3, st)
                : launch_align_io<GRAD, false, true>(K, a, io, W1, W2, w3, st);
}

// dq (B, K, E), dW1 (E, E), dW2 (E, E), dw3 (E) from the GRAD pass's partial records, fixed order
DL4SS_API int dl4ss_attn_align_finalize(const float* part, long long part_floats_, int B, int K, int T, int F,
                                        const float* q, const float* W2, float* dq, float* dW1, float* dW2,
                                        float* dw3, void* stream) {
  DL4SS_REQUIRE(part && q && W2 && dq && dW1 && dW2 && dw3 && B > 0 && K >= 1 && K <= 3 && T > 0 && F > 0);
  const int nblk = align_nblk((long long)T * F);
  DL4SS_REQUIRE(part_floats_ >= part_floats(B, K, nblk));
  return finalize(part, B, K, nblk, q, (long long)K * E, W2, dq, (long long)K * E, dW1, dW2, dw3, as_stream(stream));
}
