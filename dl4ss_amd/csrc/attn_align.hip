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
// The bf16 step's forms (align_kernel's VB / DB, dl4ss_mask_attn_align_loss_ex) change the two ends only: step 1
// reads bf16 V and widens it into the same fp32 sv, step 6 rounds dPre to bf16 on its way out, into rows of the
// GEMMs' pitch.
#include "attn_tile.h"
#include "../../include/dl4ss_align.h"

namespace {

using namespace attn_tile;

constexpr int E = 50;            // embedding size = align hidden size
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
  // the bf16 step's I/O forms of the fused passes
  const unsigned short* Vb;  // VB: (B, R, E) bf16, 4-B aligned (the Linear's EPI_TANH_BF16 output)
  unsigned short* dPreB;     // DB: (B T, ldpb) bf16, 4-B aligned; row (t, f) of b at (b T + t) ldpb + f E
  long long ldpb;            // even, >= F E
  int T, F;                  // R = T F
};

__device__ __forceinline__ float tanh_e(float x) {
  const float e = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// VB: V is read as bf16 (a.Vb; a.V unused) and converted on the way into sv; DB: dPre leaves as bf16 rows of pitch
// a.ldpb (a.dPreB; a.dPre unused).  Compile-time forms: everything between the tile load and the copy-out -- the
// fp32 arithmetic, the tiles, the order of every sum -- is one text, so the COST pass's partials on bf16 V equal,
// bit for bit, those on the same values in fp32
template <int K, int MODE, bool VB = false, bool DB = false>
__global__ __launch_bounds__(NT) void align_kernel(AlignArgs a, const float* __restrict__ W1,
                                                    const float* __restrict__ W2, const float* __restrict__ w3) {
  constexpr bool FUSED = MODE == COST || MODE == GRAD;
  constexpr bool BWD = MODE == GRAD || MODE == MBWD;
  static_assert(FUSED || K == 1, "the module-level kernels take one query per row of V");
  static_assert(FUSED || !VB, "bf16 V: the fused passes only");
  static_assert(MODE == GRAD || !DB, "bf16 dPre: the GRAD pass only");
  __shared__ __attribute__((aligned(16))) float sv[TILE * E];
  __shared__ __attribute__((aligned(16))) float su[TILE * E];
  __shared__ float sp[K * E];
  __shared__ float sw3[E];
  __shared__ float scol[BWD ? NCH * (K + 1) * E : 1];

  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  // p_k = W2 q_k, the same chain in every block of the utterance
  if (tid < K * E) {
    const int k = tid / E, aa = tid - k * E;
    const float* qk = a.q + (long long)b * a.qs + k * E;
    float acc = 0.f;
    for (int e = 0; e < E; ++e) acc = fmaf(W2[aa * E + e], qk[e], acc);
    sp[tid] = acc;
  } else if (tid < K * E + E) {
    sw3[tid - K * E] = w3[tid - K * E];
  }

  const auto [rbeg, rend] = block_rows(a.R, a.nblk);
  int pm[K];
  load_perm(FUSED ? a.perm : nullptr, b, pm);
  float cost[K * K + 1];
#pragma unroll
  for (int i = 0; i < K * K + 1; ++i) cost[i] = 0.f;
  // backward accumulators, kept over the block's tiles: the lane's 5 x 5 block of dW1 (lanes < 200)
  // and its column sums (lanes < 250): dp_k (K) and dw3
  float w1a[5][5];
  float col[K + 1];
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) w1a[i][j] = 0.f;
#pragma unroll
  for (int j = 0; j < K + 1; ++j) col[j] = 0.f;
  const int wg = tid / 100, wid = tid - wg * 100;  // dW1: row parity, block id
  const int wa0 = (wid / 10) * 5, we0 = (wid % 10) * 5;
  const int ca = tid % E, cc = tid / E;            // column sums: column, row class

  const float* Vb = VB ? nullptr : a.V + (long long)b * a.R * E;
  float* Db = (BWD && a.dPre) ? a.dPre + (long long)b * a.R * E : nullptr;

  for (int r0 = rbeg; r0 < rend; r0 += TILE) {
    const int nr = min(TILE, rend - r0);
    __syncthreads();  // the previous tile is out of sv / su (and sp, sw3 are visible on the first pass)
    if constexpr (VB) {
      // bf16 V: the tile's nr * E 16-bit words, widened to fp32 into sv.  The tile starts 4-B aligned (E even,
      // a.Vb 4-B aligned) but 16-B aligned only for some (b, r0) -- an utterance is R * 100 bytes --, so: the
      // <= 3 pairs in front of the first 16-B aligned source word singly, then 16-B loads (8 values each, written
      // as four 8-B LDS words: sv + lead is only 8-B aligned), then the <= 3 pairs left
      const unsigned short* src = a.Vb + ((long long)b * a.R + r0) * E;
      const int n = nr * E;
      const int lead = min(n, (int)((16 - ((uintptr_t)src & 15)) & 15) >> 1);
      const int n8 = (n - lead) >> 3;
      const int tail = lead + (n8 << 3);
      for (int i = tid; i < n8; i += NT) {
        const uint4 w = *reinterpret_cast<const uint4*>(src + lead + 8 * i);
        float2* d = reinterpret_cast<float2*>(sv + lead + 8 * i);
        d[0] = make_float2(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u));
        d[1] = make_float2(__uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u));
        d[2] = make_float2(__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u));
        d[3] = make_float2(__uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u));
      }
      const int np = (lead + (n - tail)) >> 1;  // head pairs [0, lead), tail pairs [tail, n)
      if (tid < np) {
        const int e = tid < (lead >> 1) ? 2 * tid : tail + 2 * (tid - (lead >> 1));
        const unsigned w = *reinterpret_cast<const unsigned*>(src + e);
        *reinterpret_cast<float2*>(sv + e) = make_float2(__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u));
      }
    } else {
      const float* src = Vb + (long long)r0 * E;
      copy_f32(sv, src, nr * E, ((uintptr_t)src & 15) == 0);
    }
    __syncthreads();
    const int r = tid;
    const bool live = r < nr;
    const int row = r0 + r;
    float* vrow = sv + r * E;
    float* urow = su + r * E;
    float s[K][E];
    float dl[K];
    if (live) {
      // ---- U = W1 v (W1 rows are wave-uniform: scalar operands)
      {
        float v[E];
#pragma unroll
        for (int e = 0; e < E; e += 2) {
          const float2 vv = *reinterpret_cast<const float2*>(vrow + e);
          v[e] = vv.x;
          v[e + 1] = vv.y;
        }
#pragma unroll 2
        for (int aa = 0; aa < E; ++aa) {
          const float* w = W1 + aa * E;
          float a0 = 0.f, a1 = 0.f;
#pragma unroll
          for (int e = 0; e < E; e += 2) {
            a0 = fmaf(w[e], v[e], a0);
            a1 = fmaf(w[e + 1], v[e + 1], a1);
          }
          urow[aa] = a0 + a1;
        }
      }
      // ---- s_k = tanh(U + p_k), logits
      float lg[K];
#pragma unroll
      for (int k = 0; k < K; ++k) lg[k] = 0.f;
#pragma unroll
      for (int aa = 0; aa < E; aa += 2) {
        const float2 uu = *reinterpret_cast<const float2*>(urow + aa);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          s[k][aa] = tanh_e(uu.x + sp[k * E + aa]);
          s[k][aa + 1] = tanh_e(uu.y + sp[k * E + aa + 1]);
          lg[k] = fmaf(sw3[aa], s[k][aa], lg[k]);
          lg[k] = fmaf(sw3[aa + 1], s[k][aa + 1], lg[k]);
        }
      }
      float m[K];
#pragma unroll
      for (int k = 0; k < K; ++k) m[k] = sigmoidf_(lg[k]);
      if constexpr (FUSED) {
        // the loss terms of dl4ss_mask_attn_loss (EvalVer.py:641,659-666)
        const float x = a.X[(long long)b * a.xs + row];
        float y[K], msum = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          msum += m[k];
          y[k] = a.Y[(long long)b * a.ys + (long long)k * a.yks + row];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int j = 0; j < K; ++j) {
            const float dd = m[k] * x - y[j];
            cost[k * K + j] = fmaf(dd, dd, cost[k * K + j]);
          }
        const float ds = msum - 1.0f;
        cost[K * K] = fmaf(ds, ds, cost[K * K]);
        if (a.mask_out || a.pred_out) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const long long o = (long long)b * a.ms + (long long)k * a.R + row;
            if (a.mask_out) a.mask_out[o] = m[k];
            if (a.pred_out) a.pred_out[o] = m[k] * x;
          }
        }
        if constexpr (MODE == GRAD) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            float yp = y[0];
#pragma unroll
            for (int j = 1; j < K; ++j) yp = pm[k] == j ? y[j] : yp;
            dl[k] = mag_dl<false>(a, k, m, x, yp, ds, 0.f);
          }
        }
      } else if constexpr (MODE == MFWD) {
        a.mask_out[(long long)b * a.ms + row] = m[0];
      } else {
        dl[0] = a.dmask[(long long)b * a.R + row] * m[0] * (1.f - m[0]);
      }
    }
    if constexpr (BWD) {
      // ---- column sums over the tile's rows: dp_k = sum_r dS_k (j < K), dw3 = sum_r sum_k dl_k s_k (j = K).
      // Round j: every live lane puts its row's values into su, lane (column ca, class cc) adds the rows
      // cc, cc + 5, ... < nr in order (address r0' * E + tid: consecutive words).  The last round leaves
      // dU = sum_k dS_k in su (K = 1: round 0 already did).
      constexpr int NROUND = K == 1 ? 2 : K + 2;
#pragma unroll
      for (int j = 0; j < NROUND; ++j) {
        // round order: dw3 first, then dS_0 .. dS_{K-1}, then (K > 1) dU
        if (live) {
#pragma unroll
          for (int aa = 0; aa < E; aa += 2) {
            float o0 = 0.f, o1 = 0.f;
            if (j == 0) {
#pragma unroll
              for (int k = 0; k < K; ++k) {
                o0 = fmaf(dl[k], s[k][aa], o0);
                o1 = fmaf(dl[k], s[k][aa + 1], o1);
              }
            } else {
#pragma unroll
              for (int k = 0; k < K; ++k) {
                if (j - 1 == k || j == K + 1) {
                  o0 += dl[k] * sw3[aa] * (1.f - s[k][aa] * s[k][aa]);
                  o1 += dl[k] * sw3[aa + 1] * (1.f - s[k][aa + 1] * s[k][aa + 1]);
                }
              }
            }
            *reinterpret_cast<float2*>(urow + aa) = make_float2(o0, o1);
          }
        }
        __syncthreads();
        if (j <= K) {
          if (tid < NCH * E) {
            float acc = col[j == 0 ? K : j - 1];
            for (int rr = cc; rr < nr; rr += NCH) acc += su[rr * E + ca];
            col[j == 0 ? K : j - 1] = acc;
          }
          if (j + 1 < NROUND) __syncthreads();  // su is rewritten by the next round
        }
      }
      // ---- dW1 += dU^T V: lane (parity wg, block wa0, we0) over the rows wg, wg + 2, ... < nr
      if (tid < 200) {
        for (int rr = wg; rr < nr; rr += 2) {
          float du[5], vv[5];
#pragma unroll
          for (int i = 0; i < 5; ++i) {
            du[i] = su[rr * E + wa0 + i];
            vv[i] = sv[rr * E + we0 + i];
          }
#pragma unroll
          for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) w1a[i][j] = fmaf(du[i], vv[j], w1a[i][j]);
        }
      }
      // ---- dV = dU W1 for the own row (registers), then over sv once every lane is done reading it
      float dv[E];
      if ((DB || Db) && live) {
#pragma unroll
        for (int e = 0; e < E; ++e) dv[e] = 0.f;
#pragma unroll 2
        for (int aa = 0; aa < E; ++aa) {
          const float du = urow[aa];
          const float* w = W1 + aa * E;
#pragma unroll
          for (int e = 0; e < E; ++e) dv[e] = fmaf(du, w[e], dv[e]);
        }
      }
      if (DB || Db) {
        __syncthreads();
        if (live) {
#pragma unroll
          for (int e = 0; e < E; e += 2) {
            if constexpr (MODE == GRAD) {  // dPre = dV (1 - V^2)
              const float2 vv = *reinterpret_cast<const float2*>(vrow + e);
              *reinterpret_cast<float2*>(vrow + e) =
                  make_float2(dv[e] * (1.f - vv.x * vv.x), dv[e + 1] * (1.f - vv.y * vv.y));
            } else {
              *reinterpret_cast<float2*>(vrow + e) = make_float2(dv[e], dv[e + 1]);
            }
          }
        }
        __syncthreads();
        if constexpr (DB) {
          // bf16 dPre: a word is a pair of sv's fp32 values, rounded to nearest even as it is read
          store_dpre_bf16<E / 2>(reinterpret_cast<unsigned*>(a.dPreB), a.ldpb, b, a.T, a.F, r0, nr, [](int i) {
            const float2 x = *reinterpret_cast<const float2*>(sv + 2 * i);
            return bf16_bits_rne(x.x) | (bf16_bits_rne(x.y) << 16);
          });
        } else {
          float* dst = Db + (long long)r0 * E;
          const int n = nr * E;
          if constexpr (MODE == GRAD) {
            copy_f32(dst, sv, n, ((uintptr_t)dst & 15) == 0);
          } else {  // the module-level dV accumulates (each element has one writer)
            for (int i = tid; i < n; i += NT) dst[i] += sv[i];
          }
        }
      }
    }
  }

  // ---- block reductions, fixed order
  if constexpr (FUSED) {
    __syncthreads();
    reduce_costs(cost, true, a.part_loss + ((long long)b * a.nblk + blockIdx.x) * (K * K + 1));
  }
  if constexpr (BWD) {
    float* pr = a.part + ((long long)b * a.nblk + blockIdx.x) * rec_floats(K);
    if (tid < 200) {
#pragma unroll
      for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) pr[wg * E * E + (wa0 + i) * E + we0 + j] = w1a[i][j];
    }
    __syncthreads();
    if (tid < NCH * E) {
#pragma unroll
      for (int j = 0; j < K + 1; ++j) scol[(cc * (K + 1) + j) * E + ca] = col[j];
    }
    __syncthreads();
    if (tid < (K + 1) * E) {  // [dp_0 .. dp_{K-1} | dw3], classes 0..4 in order
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) acc += scol[c * (K + 1) * E + tid];
      pr[W1P + tid] = acc;
    }
  }
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

long long part_floats(int B, int K, int nblk) {
  return (long long)B * nblk * rec_floats(K) + (long long)FIN_G * (E * E + E) + (long long)B * K * E;
}

template <int MODE, bool VB = false, bool DB = false>
int launch_align(int K, const AlignArgs& a, const float* W1, const float* W2, const float* w3, hipStream_t st) {
  dim3 grid(a.nblk, a.B);
  if (K == 1) hipLaunchKernelGGL((align_kernel<1, MODE, VB, DB>), grid, dim3(NT), 0, st, a, W1, W2, w3);
  if constexpr (MODE == COST || MODE == GRAD) {
    if (K == 2) hipLaunchKernelGGL((align_kernel<2, MODE, VB, DB>), grid, dim3(NT), 0, st, a, W1, W2, w3);
    if (K == 3) hipLaunchKernelGGL((align_kernel<3, MODE, VB, DB>), grid, dim3(NT), 0, st, a, W1, W2, w3);
  }
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

DL4SS_API int dl4ss_attn_align_nblk(int R) { return R < 0 ? -1 : attn_tile::nblk(R); }

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
  a.B = Bq; a.R = R; a.nblk = attn_tile::nblk(R);
  a.V = V; a.q = q; a.qs = q_stride; a.mask_out = mask; a.ms = mask_stride;
  return launch_align<MFWD>(1, a, W1, W2, w3, as_stream(stream));
}

DL4SS_API int dl4ss_attn_align_bwd(const float* V, const float* q, int q_stride, const float* W1, const float* W2,
                                   const float* w3, const float* dmask, int Bq, int R, int E_, float* dV, float* part,
                                   long long part_floats_, float* dq, float* dW1, float* dW2, float* dw3,
                                   void* stream) {
  DL4SS_REQUIRE(V && q && W1 && W2 && w3 && dmask && part && dq && dW1 && dW2 && dw3);
  DL4SS_REQUIRE(Bq > 0 && R > 0 && E_ == E && q_stride >= E);
  const int nblk = attn_tile::nblk(R);
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
  const int nblk = attn_tile::nblk(R);
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
  const int nblk = attn_tile::nblk(R);
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
  a.Vb = static_cast<const unsigned short*>(V_bf16);
  a.dPreB = static_cast<unsigned short*>(dPre_bf16); a.ldpb = dpre_bf16_ld; a.T = T; a.F = F;
  hipStream_t st = as_stream(stream);
  if (pass == 0)
    return V_bf16 ? launch_align<COST, true, false>(K, a, W1, W2, w3, st) : launch_align<COST>(K, a, W1, W2, w3, st);
  if (dPre) return launch_align<GRAD>(K, a, W1, W2, w3, st);  // fp32 V, fp32 dPre: dl4ss_mask_attn_align_loss
  return V_bf16 ? launch_align<GRAD, true, true>(K, a, W1, W2, w3, st)
                : launch_align<GRAD, false, true>(K, a, W1, W2, w3, st);
}

// dq (B, K, E), dW1 (E, E), dW2 (E, E), dw3 (E) from the GRAD pass's partial records, fixed order
DL4SS_API int dl4ss_attn_align_finalize(const float* part, long long part_floats_, int B, int K, int T, int F,
                                        const float* q, const float* W2, float* dq, float* dW1, float* dW2,
                                        float* dw3, void* stream) {
  DL4SS_REQUIRE(part && q && W2 && dq && dW1 && dW2 && dw3 && B > 0 && K >= 1 && K <= 3 && T > 0 && F > 0);
  const int nblk = attn_tile::nblk((long long)T * F);
  DL4SS_REQUIRE(part_floats_ >= part_floats(B, K, nblk));
  return finalize(part, B, K, nblk, q, (long long)K * E, W2, dq, (long long)K * E, dW1, dW2, dw3, as_stream(stream));
}
