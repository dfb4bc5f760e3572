// The body of align_kernel and align_io_kernel (attn_align.hip), included inside both kernel definitions so that
// each compiles from the same text.  In scope: the template parameters K, MODE, the kernel arguments `a`
// (AlignArgs), W1, W2, w3, `constexpr bool VB, DB` and `io` (AlignIO; unused when VB and DB are false).  VB: V is
// read as bf16 (io.Vb) and converted on the way into sv; DB: dPre leaves as bf16 rows of pitch io.ldpb
// (io.dPreB).  Everything between the tile load and the copy-out -- the fp32 arithmetic, the tiles, the order of
// every sum -- is one text for all forms.  Not a header: no guard, no declarations.
  constexpr bool FUSED = MODE == COST || MODE == GRAD;
  constexpr bool BWD = MODE == GRAD || MODE == MBWD;
  static_assert(FUSED || K == 1, "the module-level kernels take one query per row of V");
  static_assert(FUSED || !VB, "bf16 V: the fused passes only");
  static_assert(MODE == GRAD || !DB, "bf16 dPre: the GRAD pass only");
  __shared__ __attribute__((aligned(16))) float sv[TILE * E];
  __shared__ __attribute__((aligned(16))) float su[TILE * E];
  __shared__ float sp[K * E];
  __shared__ float sw3[E];
  __shared__ float sred[NT / 64][K * K + 1];
  __shared__ float scol[BWD ? NCH * (K + 1) * E : 1];

  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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

  const int per = (a.R + a.nblk - 1) / a.nblk;
  const int rbeg = blockIdx.x * per;
  const int rend = min(a.R, rbeg + per);

  int pm[K];
#pragma unroll
  for (int k = 0; k < K; ++k) pm[k] = (FUSED && a.perm) ? a.perm[b * K + k] : k;
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
      // io.Vb 4-B aligned) but 16-B aligned only for some (b, r0) -- an utterance is R * 100 bytes --, so: the
      // <= 3 pairs in front of the first 16-B aligned source word singly, then 16-B loads (8 values each, written
      // as four 8-B LDS words: sv + lead is only 8-B aligned), then the <= 3 pairs left
      const unsigned short* src = io.Vb + ((long long)b * a.R + r0) * E;
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
      const int n = nr * E;
      if (((uintptr_t)src & 15) == 0) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += NT) reinterpret_cast<float4*>(sv)[i] = reinterpret_cast<const float4*>(src)[i];
        for (int i = (n4 << 2) + tid; i < n; i += NT) sv[i] = src[i];
      } else {
        for (int i = tid; i < n; i += NT) sv[i] = src[i];
      }
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
            const float dm = 2.f * a.s1 * (m[k] * x - yp) * x + 2.f * a.s2 * ds;
            dl[k] = dm * m[k] * (1.f - m[k]);
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
          // bf16 dPre, rounded to nearest even, into rows (b T + t) of the (B T, ldpb) matrix the Linear's backward
          // GEMMs read: row (t, f) lives at t ldpb + f E, so the tile's values of frame t are one contiguous run
          // and the tile is one run per frame it touches; the columns >= F E of a row are never written.  In
          // 32-bit words (a pair of values; E, ldpb and the matrix are even): each run goes out as 16-B stores
          // from its first 16-B aligned destination word (four words = eight fp32 values of sv), its <= 3 head
          // and <= 3 tail words singly, as attn_q4_kernel writes its dPre
          constexpr int EP = E / 2;
          unsigned* const dw = reinterpret_cast<unsigned*>(io.dPreB);
          const long long rowb = (long long)b * io.T;
          const int ntot = nr * EP;
          for (int t = r0 / io.F, sw = 0; sw < ntot; ++t) {
            const int ew = min(ntot, ((t + 1) * io.F - r0) * EP);  // end of frame t's words in the tile
            unsigned* dst = dw + ((rowb + t) * io.ldpb >> 1) + (long long)(r0 - t * io.F) * EP;  // + word of the tile
            const int lead = (int)((4 - (((uintptr_t)(dst + sw)) >> 2)) & 3);  // words before the first aligned one
            const int i0 = min(ew, sw + lead);
            const int nq = (ew - i0) >> 2;
            auto word = [&](int i) {
              const float2 x = *reinterpret_cast<const float2*>(sv + 2 * i);
              return bf16_bits_rne(x.x) | (bf16_bits_rne(x.y) << 16);
            };
            for (int q = tid; q < nq; q += NT) {
              const int i = i0 + 4 * q;
              *reinterpret_cast<uint4*>(dst + i) = make_uint4(word(i), word(i + 1), word(i + 2), word(i + 3));
            }
            const int te = i0 + 4 * nq;  // tail words [te, ew), head words [sw, i0)
            if (tid < i0 - sw) dst[sw + tid] = word(sw + tid);
            if (tid >= 4 && tid - 4 < ew - te) dst[te + tid - 4] = word(te + tid - 4);
            sw = ew;
          }
        } else {
          float* dst = Db + (long long)r0 * E;
          const int n = nr * E;
          if constexpr (MODE == GRAD) {
            if (((uintptr_t)dst & 15) == 0) {
              const int n4 = n >> 2;
              for (int i = tid; i < n4; i += NT)
                reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(sv)[i];
              for (int i = (n4 << 2) + tid; i < n; i += NT) dst[i] = sv[i];
            } else {
              for (int i = tid; i < n; i += NT) dst[i] = sv[i];
            }
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
#pragma unroll
    for (int i = 0; i < K * K + 1; ++i) {
      const float t = wave_sum(cost[i]);
      if (lane == 0) sred[wave][i] = t;
    }
    __syncthreads();
    float* pl = a.part_loss + ((long long)b * a.nblk + blockIdx.x) * (K * K + 1);
    if (tid < K * K + 1) pl[tid] = sred[0][tid] + sred[1][tid] + sred[2][tid] + sred[3][tid];
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
