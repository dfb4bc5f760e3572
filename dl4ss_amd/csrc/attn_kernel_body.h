// The body of attn_kernel and attn_adv_kernel (attn_loss.hip), included inside both kernel definitions so
// that each compiles from the same text.  In scope: the template parameters E, K, CRM, GRAD, VB, the kernel
// argument `a` (AttnArgs), `constexpr bool ADV` and `const float* gext` (the adversarial GRAD pass's gradient
// at the prediction, (B, K, T*F); unused when ADV is false).  Not a header: no guard, no declarations.
  constexpr int QW = CRM ? 2 * E : E;
  constexpr int NC = CRM ? 2 : 1;  // components per bin
  __shared__ __attribute__((aligned(16))) float sv[TILE * E];
  __shared__ float sq[K * QW];
  __shared__ float sred[NT / 64][K * K + 1];

  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < K * QW; i += NT) sq[i] = a.q[(long long)b * K * QW + i];

  // this block's row range
  const int per = (a.rows_per_b + a.nblk - 1) / a.nblk;
  const int rbeg = blockIdx.x * per;
  const int rend = min(a.rows_per_b, rbeg + per);

  int pm[K];
#pragma unroll
  for (int k = 0; k < K; ++k) pm[k] = a.perm ? a.perm[b * K + k] : k;

  float cost[K * K + 1];
#pragma unroll
  for (int i = 0; i < K * K + 1; ++i) cost[i] = 0.f;
  __shared__ float sdl[GRAD ? TILE * K * NC : 1];  // dL/dlogit per tile row
  float dqa[2] = {0.f, 0.f};  // dq[j] for j = tid, tid + 256 (j < K*QW)
  const float* Vb = a.V + (long long)b * a.rows_per_b * E;
  float* Db = (GRAD && a.dPre) ? a.dPre + (long long)b * a.rows_per_b * E : nullptr;

  for (int r0 = rbeg; r0 < rend; r0 += TILE) {
    const int nr = min(TILE, rend - r0);
    __syncthreads();  // previous tile fully consumed (and sq visible on first pass)
    // coalesced stage of nr rows (nr*E floats, 16-B aligned when r0*E*4 % 16 == 0); bf16 V:
    // 4-B pairs (E even), widened to fp32 in LDS
    if constexpr (VB) {
      const unsigned* src = reinterpret_cast<const unsigned*>(a.Vb + ((long long)b * a.rows_per_b + r0) * E);
      const int n2 = nr * E / 2;
      // every load of the tile issued before the first LDS store (a load -> store loop
      // kept one 4-B load per thread in flight)
      constexpr int NW = (TILE * E / 2 + NT - 1) / NT;
      unsigned w[NW];
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const int i = tid + q * NT;
        w[q] = i < n2 ? src[i] : 0u;
      }
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const int i = tid + q * NT;
        if (i < n2)
          reinterpret_cast<float2*>(sv)[i] = make_float2(__uint_as_float(w[q] << 16), __uint_as_float(w[q] & 0xFFFF0000u));
      }
    } else {
      const float* src = Vb + (long long)r0 * E;
      const int n = nr * E;
      if ((((long long)r0 * E) & 3) == 0) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += NT) reinterpret_cast<float4*>(sv)[i] = reinterpret_cast<const float4*>(src)[i];
        for (int i = (n4 << 2) + tid; i < n; i += NT) sv[i] = src[i];
      } else {
        for (int i = tid; i < n; i += NT) sv[i] = src[i];
      }
    }
    __syncthreads();
    const int r = tid;
    if (r < nr) {
      const int row = r0 + r;
      const float* v = sv + r * E;
      float lg[K * NC];
#pragma unroll
      for (int i = 0; i < K * NC; ++i) lg[i] = 0.f;
#pragma unroll
      for (int e = 0; e < E; e += 2) {
        const float2 vv = *reinterpret_cast<const float2*>(v + e);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            lg[k * NC + c] = fmaf(vv.x, sq[k * QW + c * E + e], lg[k * NC + c]);
            lg[k * NC + c] = fmaf(vv.y, sq[k * QW + c * E + e + 1], lg[k * NC + c]);
          }
      }
      float dl[K * NC];  // dL/dlogit
      if constexpr (!CRM) {
        const float x = a.X[(long long)b * a.xs + row];
        float m[K], y[K], msum = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          m[k] = sigmoidf_(lg[k]);
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
            const long long o = ((long long)b * K + k) * a.rows_per_b + row;
            if (a.mask_out) a.mask_out[o] = m[k];
            if (a.pred_out) a.pred_out[o] = m[k] * x;
          }
        }
        if constexpr (GRAD) {
          float yp[K];
#pragma unroll
          for (int k = 0; k < K; ++k) {
            yp[k] = y[0];
#pragma unroll
            for (int j = 1; j < K; ++j) yp[k] = pm[k] == j ? y[j] : yp[k];
          }
#pragma unroll
          for (int k = 0; k < K; ++k) {
            float dm;
            if constexpr (ADV)
              dm = (2.f * a.s1 * (m[k] * x - yp[k]) + gext[((long long)b * K + k) * a.rows_per_b + row]) * x +
                   2.f * a.s2 * ds;
            else
              dm = 2.f * a.s1 * (m[k] * x - yp[k]) * x + 2.f * a.s2 * ds;
            dl[k] = dm * m[k] * (1.f - m[k]);
          }
        }
      } else {
        const float2 x = *reinterpret_cast<const float2*>(a.X + 2 * ((long long)b * a.xs + row));
        float2 p[K], y[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          // cRM_EvalVer.py:269 (10 tanh) and :688 (inverse compression), fp32 as the reference
          const float mcr = 10.f * tanhf(lg[k * 2]);
          const float mci = 10.f * tanhf(lg[k * 2 + 1]);
          const float mr = -10.f * logf((10.f - mcr) / (10.f + mcr));
          const float mi = -10.f * logf((10.f - mci) / (10.f + mci));
          p[k] = make_float2(mr * x.x - mi * x.y, mr * x.y + mi * x.x);
          y[k] = *reinterpret_cast<const float2*>(a.Y + 2 * ((long long)b * a.ys + (long long)k * a.yks + row));
          if (a.mask_out) {
            const long long o = 2 * (((long long)b * K + k) * a.rows_per_b + row);
            a.mask_out[o] = mr;
            a.mask_out[o + 1] = mi;
          }
          if (a.pred_out) {
            const long long o = 2 * (((long long)b * K + k) * a.rows_per_b + row);
            a.pred_out[o] = p[k].x;
            a.pred_out[o + 1] = p[k].y;
          }
          if constexpr (GRAD) {
            // d(M)/d(logit) through the same fp32 chain: dM/dMc * dMc/dl
            const float dmc_r = 10.f * (1.f / (10.f - mcr) + 1.f / (10.f + mcr));
            const float dmc_i = 10.f * (1.f / (10.f - mci) + 1.f / (10.f + mci));
            dl[k * 2] = dmc_r * (10.f * (1.f - (mcr * 0.1f) * (mcr * 0.1f)));
            dl[k * 2 + 1] = dmc_i * (10.f * (1.f - (mci * 0.1f) * (mci * 0.1f)));
          }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int j = 0; j < K; ++j) {
            const float dr = p[k].x - y[j].x, di = p[k].y - y[j].y;
            cost[k * K + j] = fmaf(dr, dr, fmaf(di, di, cost[k * K + j]));
          }
        if constexpr (GRAD) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            float2 yp = y[0];
#pragma unroll
            for (int j = 1; j < K; ++j) yp = pm[k] == j ? y[j] : yp;
            const float gr = 2.f * a.s1 * (p[k].x - yp.x), gi = 2.f * a.s1 * (p[k].y - yp.y);
            // P = M (x) X: dMr = gr xr + gi xi ; dMi = -gr xi + gi xr
            const float dmr = gr * x.x + gi * x.y;
            const float dmi = -gr * x.y + gi * x.x;
            dl[k * 2] *= dmr;
            dl[k * 2 + 1] *= dmi;
          }
        }
      }
      if constexpr (GRAD) {
#pragma unroll
        for (int i = 0; i < K * NC; ++i) sdl[r * K * NC + i] = dl[i];
      }
    } else if (GRAD) {
#pragma unroll
      for (int i = 0; i < K * NC; ++i) sdl[r * K * NC + i] = 0.f;
    }
    if constexpr (GRAD) {
      __syncthreads();
      // dq[k][c*E+e] += sum_r dl[r][k*NC+c] V[r][e]   (lanes along e: conflict-free)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = tid + NT * h;
        if (j < K * QW) {
          const int k = j / QW, ce = j % QW, c = ce / E, e = ce % E;
          float acc = 0.f;
          for (int rr = 0; rr < nr; ++rr) acc = fmaf(sdl[rr * K * NC + k * NC + c], sv[rr * E + e], acc);
          dqa[h] += acc;
        }
      }
      __syncthreads();
      // dV[e] = sum_k dl_k q_k[e] ; dPre = dV (1 - V^2), written in place over the own row
      if (r < nr) {
        float* v = sv + r * E;
        float dl[K * NC];
#pragma unroll
        for (int i = 0; i < K * NC; ++i) dl[i] = sdl[r * K * NC + i];
#pragma unroll
        for (int e = 0; e < E; e += 2) {
          const float2 vv = *reinterpret_cast<const float2*>(v + e);
          float g0 = 0.f, g1 = 0.f;
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              const float d = dl[k * NC + c];
              g0 = fmaf(d, sq[k * QW + c * E + e], g0);
              g1 = fmaf(d, sq[k * QW + c * E + e + 1], g1);
            }
          *reinterpret_cast<float2*>(v + e) = make_float2(g0 * (1.f - vv.x * vv.x), g1 * (1.f - vv.y * vv.y));
        }
      }
    }
    if (GRAD && a.dPreB) {
      // bf16 dPre for the Linear's backward GEMMs: pairs (e, e+1) as one 4-B store into
      // row (b*T + t) of the padded bf16 matrix (E, F*E offsets and ldpb are even)
      __syncthreads();
      for (int i = tid; i < nr * E / 2; i += NT) {
        const int rl = (2 * i) / E, e = (2 * i) % E;
        const int row = r0 + rl;
        const int t = row / a.F, f = row - t * a.F;
        __hip_bfloat162 v2 = __float22bfloat162_rn(make_float2(sv[2 * i], sv[2 * i + 1]));
        a.dPreB[(((long long)b * a.T + t) * a.ldpb + (long long)f * E + e) >> 1] = *reinterpret_cast<unsigned*>(&v2);
      }
    } else if constexpr (GRAD) {
      __syncthreads();
      float* dst = Db + (long long)r0 * E;
      const int n = nr * E;
      if ((((long long)r0 * E) & 3) == 0) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += NT) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(sv)[i];
        for (int i = (n4 << 2) + tid; i < n; i += NT) dst[i] = sv[i];
      } else {
        for (int i = tid; i < n; i += NT) dst[i] = sv[i];
      }
    }
  }

  // ---- block reductions (fixed order: wave shuffle, then waves 0..3)
  __syncthreads();
#pragma unroll
  for (int i = 0; i < K * K + 1; ++i) {
    const float s = wave_sum(cost[i]);
    if (lane == 0) sred[wave][i] = s;
  }
  __syncthreads();
  float* pl = a.part_loss + ((long long)b * a.nblk + blockIdx.x) * (K * K + 1);
  if (tid < K * K + 1) pl[tid] = sred[0][tid] + sred[1][tid] + sred[2][tid] + sred[3][tid];
  if constexpr (GRAD) {
    float* pd = a.part_dq + ((long long)b * a.nblk + blockIdx.x) * K * QW;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (tid + NT * h < K * QW) pd[tid + NT * h] = dqa[h];
  }
