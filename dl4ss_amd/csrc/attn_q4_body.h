// The body of attn_q4_kernel and attn_q4_adv_kernel (attn_loss.hip), included inside both kernel definitions
// so that each compiles from the same text.  In scope: the template parameters E, K, GRAD, VF, CRM, the kernel
// argument `a` (AttnArgs), `constexpr bool ADV` and `const float* gext` (the adversarial GRAD pass's gradient
// at the prediction, (B, K, T*F); unused when ADV is false).  Not a header: no guard, no declarations.
  // CRM (round 5): the complex-ratio-mask path (cRM_EvalVer.py:259-271, 688, 720-743) -- each row
  // has NC = 2 logits per query (the re / im halves of the 2E-wide query), the inverse-compressed mask
  // M, the complex prediction P = M (x) X and its squared error, as attn_kernel computes them (the same
  // fp32 tanhf / logf chain) -- on the quad layout; only the logits' summation order differs.
  constexpr int NC = CRM ? 2 : 1;        // logits per (row, query)
  constexpr int QW = NC * E;             // query width
  constexpr int EP = E / 2;              // bf16 pairs per row
  constexpr int NWL = (EP + 3) / 4;      // pairs per lane
  constexpr int NQ = NT / 4;             // quads per block
  constexpr int RPQ = TILE / NQ;         // rows per quad per tile
  constexpr int WPR = VF ? E : EP;       // 4-B words of V per row
  constexpr int NCH = (TILE * WPR + 3) / 4 + 1;  // 16-B chunks of a tile, misaligned start included
  constexpr int NCHP = (NCH + 63) / 64 * 64;     // whole 1-KB DMA instructions
  __shared__ __attribute__((aligned(16))) unsigned sv[NCHP * 4];
  __shared__ __attribute__((aligned(16))) unsigned sdp[VF && GRAD ? TILE * EP : 1];
  __shared__ float sred[NT / 64][K * K + 1];
  __shared__ float sdq[GRAD ? NT / 64 * K * QW : 1];

  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = tid & 3, qd = tid >> 2;
  // this lane's q values (zero for the pair slots past EP)
  float qv[K][NC][NWL][2];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < NWL; ++i) {
        const int w = j + 4 * i;
        const float* qk = a.q + ((long long)b * K + k) * QW + c * E;
        qv[k][c][i][0] = w < EP ? qk[2 * w] : 0.f;
        qv[k][c][i][1] = w < EP ? qk[2 * w + 1] : 0.f;
      }
  const int per = (a.rows_per_b + a.nblk - 1) / a.nblk;
  const int rbeg = blockIdx.x * per;
  const int rend = min(a.rows_per_b, rbeg + per);
  int pm[K];
#pragma unroll
  for (int k = 0; k < K; ++k) pm[k] = a.perm ? a.perm[b * K + k] : k;
  float cost[K * K + 1];
#pragma unroll
  for (int i = 0; i < K * K + 1; ++i) cost[i] = 0.f;
  float dq[GRAD ? K : 1][GRAD ? NC : 1][GRAD ? NWL : 1][2];
  if constexpr (GRAD) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < NWL; ++i) dq[k][c][i][0] = dq[k][c][i][1] = 0.f;
  }
  const unsigned* Vw = VF ? reinterpret_cast<const unsigned*>(a.V) : reinterpret_cast<const unsigned*>(a.Vb);
  const long long totw = (long long)a.B * a.rows_per_b * WPR;

  for (int r0 = rbeg; r0 < rend; r0 += TILE) {
    const int nr = min(TILE, rend - r0);
    // issue this tile's loads: X and the targets of the quad's rows (cRM: [re, im]), then V by 16-B chunks
    float xr[RPQ][NC], yr[RPQ][K][NC];
#pragma unroll
    for (int s = 0; s < RPQ; ++s) {
      const int r = qd + NQ * s;
      const int row = r0 + (r < nr ? r : 0);
#pragma unroll
      for (int c = 0; c < NC; ++c) xr[s][c] = a.X[((long long)b * a.xs + row) * NC + c];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < NC; ++c) yr[s][k][c] = a.Y[((long long)b * a.ys + (long long)k * a.yks + row) * NC + c];
    }
    float ge[ADV ? RPQ : 1][ADV ? K : 1];  // ADV: the rows' gradient at the prediction, loaded with X and Y
    if constexpr (ADV) {
#pragma unroll
      for (int s = 0; s < RPQ; ++s) {
        const int r = qd + NQ * s;
        const int row = r0 + (r < nr ? r : 0);
#pragma unroll
        for (int k = 0; k < K; ++k) ge[s][k] = gext[((long long)b * K + k) * a.rows_per_b + row];
      }
    }
    const long long w0 = ((long long)b * a.rows_per_b + r0) * WPR;
    const int off = (int)(w0 & 3);  // (VF: even -- E is -- so every pair is an aligned float2)
    const long long wa = w0 - off;
    const int nch = (off + nr * WPR + 3) >> 2;
    __syncthreads();  // the previous tile's rows and dPre copy-out are done with sv
    // V by LDS-DMA: wave instruction p moves chunks 64p .. 64p + 63 (1 KB) into sv + 256p words
    int tail = -1;
    for (int p = wave; p * 64 < nch; p += NT / 64) {
      const int c = p * 64 + lane;
      const long long gw = wa + 4LL * c;
      const bool whole = c < nch && gw + 4 <= totw;
      if (c < nch && !whole) tail = c;
      __builtin_amdgcn_global_load_lds(whole ? (const void*)(Vw + gw) : (const void*)g_attn_zero,
                                       (attn_lds_void*)(sv + 256 * p), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tail >= 0) {  // the buffer's last chunk, partly past its end: the valid words by plain loads
      const long long gw = wa + 4LL * tail;
      for (int q = 0; q < 4 && gw + q < totw; ++q) sv[4 * tail + q] = Vw[gw + q];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < RPQ; ++s) {
      const int r = qd + NQ * s;
      if (r < nr) {  // quad-uniform
        const int row = r0 + r;
        unsigned* v = VF ? sdp + r * EP + j : sv + off + r * EP + j;  // (VF: the dPre pairs' LDS words)
        float vxs[NWL], vys[NWL];
        if constexpr (VF) {
          const float2* vf = reinterpret_cast<const float2*>(sv + off + r * E) + j;
#pragma unroll
          for (int i = 0; i < NWL; ++i) {
            const float2 p = (j + 4 * i < EP) ? vf[4 * i] : make_float2(0.f, 0.f);
            vxs[i] = p.x;
            vys[i] = p.y;
          }
        } else {
#pragma unroll
          for (int i = 0; i < NWL; ++i) {
            const unsigned w = (j + 4 * i < EP) ? v[4 * i] : 0u;
            vxs[i] = __uint_as_float(w << 16);
            vys[i] = __uint_as_float(w & 0xFFFF0000u);
          }
        }
        float lg[K][NC];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int c = 0; c < NC; ++c) lg[k][c] = 0.f;
#pragma unroll
        for (int i = 0; i < NWL; ++i) {
          const float vx = vxs[i], vy = vys[i];
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              lg[k][c] = fmaf(vx, qv[k][c][i][0], lg[k][c]);
              lg[k][c] = fmaf(vy, qv[k][c][i][1], lg[k][c]);
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            lg[k][c] += quad_xor1(lg[k][c]);
            lg[k][c] += quad_xor2(lg[k][c]);
          }
        float dl[K][NC];  // dL/dlogit (GRAD)
        if constexpr (!CRM) {
          const float x = xr[s][0];
          float m[K], msum = 0.f;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            m[k] = sigmoidf_(lg[k][0]);
            msum += m[k];
          }
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int jj = 0; jj < K; ++jj) {
              const float dd = m[k] * x - yr[s][jj][0];
              cost[k * K + jj] = fmaf(dd, dd, cost[k * K + jj]);
            }
          const float ds = msum - 1.0f;
          cost[K * K] = fmaf(ds, ds, cost[K * K]);
          if ((a.mask_out || a.pred_out) && j == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
              const long long o = ((long long)b * K + k) * a.rows_per_b + row;
              if (a.mask_out) a.mask_out[o] = m[k];
              if (a.pred_out) a.pred_out[o] = m[k] * x;
            }
          }
          if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
              float yp = yr[s][0][0];
#pragma unroll
              for (int jj = 1; jj < K; ++jj) yp = pm[k] == jj ? yr[s][jj][0] : yp;
              float dm;
              if constexpr (ADV)
                dm = (2.f * a.s1 * (m[k] * x - yp) + ge[s][k]) * x + 2.f * a.s2 * ds;
              else
                dm = 2.f * a.s1 * (m[k] * x - yp) * x + 2.f * a.s2 * ds;
              dl[k][0] = dm * m[k] * (1.f - m[k]);
            }
          }
        } else {
          const float2 x = make_float2(xr[s][0], xr[s][1]);
          float2 p[K];
#pragma unroll
          for (int k = 0; k < K; ++k) {
            // cRM_EvalVer.py:269 (10 tanh) and :688 (inverse compression), fp32 as the reference
            const float mcr = 10.f * tanhf(lg[k][0]);
            const float mci = 10.f * tanhf(lg[k][1]);
            const float mr = -10.f * logf((10.f - mcr) / (10.f + mcr));
            const float mi = -10.f * logf((10.f - mci) / (10.f + mci));
            p[k] = make_float2(mr * x.x - mi * x.y, mr * x.y + mi * x.x);
            if (j == 0) {
              const long long o = 2 * (((long long)b * K + k) * a.rows_per_b + row);
              if (a.mask_out) { a.mask_out[o] = mr; a.mask_out[o + 1] = mi; }
              if (a.pred_out) { a.pred_out[o] = p[k].x; a.pred_out[o + 1] = p[k].y; }
            }
            if constexpr (GRAD) {
              // d(M)/d(logit) through the same fp32 chain: dM/dMc * dMc/dl
              const float dmc_r = 10.f * (1.f / (10.f - mcr) + 1.f / (10.f + mcr));
              const float dmc_i = 10.f * (1.f / (10.f - mci) + 1.f / (10.f + mci));
              dl[k][0] = dmc_r * (10.f * (1.f - (mcr * 0.1f) * (mcr * 0.1f)));
              dl[k][1] = dmc_i * (10.f * (1.f - (mci * 0.1f) * (mci * 0.1f)));
            }
          }
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int jj = 0; jj < K; ++jj) {
              const float dr = p[k].x - yr[s][jj][0], di = p[k].y - yr[s][jj][1];
              cost[k * K + jj] = fmaf(dr, dr, fmaf(di, di, cost[k * K + jj]));
            }
          if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
              float2 yp = make_float2(yr[s][0][0], yr[s][0][1]);
#pragma unroll
              for (int jj = 1; jj < K; ++jj) yp = pm[k] == jj ? make_float2(yr[s][jj][0], yr[s][jj][1]) : yp;
              const float gr = 2.f * a.s1 * (p[k].x - yp.x), gi = 2.f * a.s1 * (p[k].y - yp.y);
              // P = M (x) X: dMr = gr xr + gi xi ; dMi = -gr xi + gi xr
              dl[k][0] *= gr * x.x + gi * x.y;
              dl[k][1] *= -gr * x.y + gi * x.x;
            }
          }
        }
        if constexpr (GRAD) {
          // dV[e] = sum_{k,c} dl_kc q_kc[e]; dPre = dV (1 - V^2) as bf16 over the lane's own words;
          // dq_kc[e] += dl_kc V[e]
#pragma unroll
          for (int i = 0; i < NWL; ++i) {
            const float vx = vxs[i], vy = vys[i];
            float g0 = 0.f, g1 = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
              for (int c = 0; c < NC; ++c) {
                g0 = fmaf(dl[k][c], qv[k][c][i][0], g0);
                g1 = fmaf(dl[k][c], qv[k][c][i][1], g1);
                dq[k][c][i][0] = fmaf(dl[k][c], vx, dq[k][c][i][0]);
                dq[k][c][i][1] = fmaf(dl[k][c], vy, dq[k][c][i][1]);
              }
            __hip_bfloat162 o2 = __float22bfloat162_rn(make_float2(g0 * (1.f - vx * vx), g1 * (1.f - vy * vy)));
            if (j + 4 * i < EP) v[4 * i] = *reinterpret_cast<unsigned*>(&o2);
          }
        }
      }
    }
    if constexpr (GRAD) {
      // bf16 dPre rows (b*T + t) of the padded matrix: the tile's words [s, e) of frame t go to
      // words (r0 - t F) EP + i of that row, one contiguous segment per frame (at most 3 here).
      // Rows start 16-B aligned (ldpb % 8 == 0), so each segment is written as 16-B stores from its
      // first 16-B aligned destination word on (four LDS words each: the source is only 4-B
      // aligned), with its <= 3 head and <= 3 tail words stored singly: a quarter of the store
      // instructions of a word-per-lane copy.
      __syncthreads();
      const int t0 = r0 / a.F;
      const long long rowb = (long long)b * a.T;
      const int ntot = nr * EP;
      for (int t = t0, sw = 0; sw < ntot; ++t) {
        const int ew = min(ntot, ((t + 1) * a.F - r0) * EP);  // end of frame t's words in the tile
        unsigned* dst = a.dPreB + ((rowb + t) * a.ldpb >> 1) + (long long)(r0 - t * a.F) * EP;  // + i
        const int lead = (int)((4 - (((uintptr_t)(dst + sw)) >> 2)) & 3);  // words before the first aligned one
        const int i0 = min(ew, sw + lead);
        const int nq = (ew - i0) >> 2;
        const unsigned* so = VF ? sdp : sv + off;  // the tile's dPre words
        for (int q = tid; q < nq; q += NT) {
          const int i = i0 + 4 * q;
          *reinterpret_cast<uint4*>(dst + i) = make_uint4(so[i], so[i + 1], so[i + 2], so[i + 3]);
        }
        const int te = i0 + 4 * nq;  // tail words [te, ew), head words [sw, i0)
        if (tid < i0 - sw) dst[sw + tid] = so[sw + tid];
        if (tid >= 4 && tid - 4 < ew - te) dst[te + tid - 4] = so[te + tid - 4];
        sw = ew;
      }
    }
  }

  // ---- block reductions (fixed order: lane trees, then waves 0..3); costs from lane 0 of each quad
  __syncthreads();
#pragma unroll
  for (int i = 0; i < K * K + 1; ++i) {
    const float s = wave_sum(j == 0 ? cost[i] : 0.f);
    if (lane == 0) sred[wave][i] = s;
  }
  if constexpr (GRAD) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < NWL; ++i)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            float s = dq[k][c][i][h];
#pragma unroll
            for (int o = 4; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
            const int w = lane + 4 * i;  // lanes 0..3 hold the wave's sums of pairs j + 4i
            if (lane < 4 && w < EP) sdq[(wave * K + k) * QW + c * E + 2 * w + h] = s;
          }
  }
  __syncthreads();
  float* pl = a.part_loss + ((long long)b * a.nblk + blockIdx.x) * (K * K + 1);
  if (tid < K * K + 1) pl[tid] = sred[0][tid] + sred[1][tid] + sred[2][tid] + sred[3][tid];
  if constexpr (GRAD) {
    float* pd = a.part_dq + ((long long)b * a.nblk + blockIdx.x) * K * QW;
    for (int i = tid; i < K * QW; i += NT)
      pd[i] = sdq[0 * K * QW + i] + sdq[1 * K * QW + i] + sdq[2 * K * QW + i] + sdq[3 * K * QW + i];
  }
