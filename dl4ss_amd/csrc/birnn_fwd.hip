// Generic forward recurrence of the persistent BiLSTM / BiGRU (one-value granules; fp32 parity mode,
// bf16 MFMA mode, the large-H instantiations) and its launch selection.  Decomposition, hand-off and
// wave roles: birnn_common.h.
#include "birnn_common.h"

namespace dl4ss_rnn {

// MF = false: exact fp32 matvec on the VALU (the parity mode); W_hh slice in fp32
//      registers, k split over KP thread parts, partial sums combined by the cell thread.
// MF = true: bf16 MFMA matvec (v_mfma_f32_16x16x32_bf16, fp32 accumulate; the
//      throughput mode): wave m owns the 16-row tile m of W_hh (bf16 A fragments in
//      registers for all K), h staged in LDS as bf16 [batch][k] (the B operand), one
//      MFMA chain per wave -- no partial sums at all.
// HARD = true: Keras 1's LSTM cell (DL4SS_RNN_HARD_GATES): the i, f and o gates are hard_sigmoid of
//      the same pre-activation (one FMA and a clamp, hsig of birnn_common.h) instead of the logistic
//      function; g, c and h are unchanged.  fp32 LSTM, runtime-bounds instantiations only.
template <int CELL, int BC, int KPL_T, bool MF, int HM = HMAX, bool HARD = false>
__global__ __launch_bounds__(NT, 1) void rnn_fwd_kernel(RnnArgs a) {
  static_assert(!HARD || (CELL == CELL_LSTM && !MF && KPL_T == 0), "hard gates: fp32 LSTM, runtime bounds");
  constexpr int WN = MF ? 1 : (KPL_T > 0 ? KPL_T : WMAX);  // fp32 weights per thread (compile-time)
  constexpr int NGATE = CELL == CELL_LSTM ? 4 : 3;
  constexpr int KSMAX = HM / 32;
  const int H = a.H, T = a.T, J = a.J;
  const int R = NGATE * J;
  const int ngroups = 2 * a.nchunk;
  int group, w;
  group_of(blockIdx.x, a.NG, ngroups, group, w);
  const int d = group / a.nchunk, chunk = group % a.nchunk;
  const int b0 = chunk * BC;
  const int j0 = w * J;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int GH = NGATE * H;
  const int MT = (R + 15) / 16;
  constexpr int SHB = shb_stride(HM);  // bf16 row stride of the MFMA B image (k >= H stays zero)

  extern __shared__ __attribute__((aligned(16))) float smem[];
  // fp32 path: sh [BC][HP], spart [KP][BC][R]; MFMA path: shb bf16 [16][SHB], sgate [BC][MT*16]
  // (region lengths: fwd_sh_n / fwd_spart_n / fwd_shb_n / fwd_sgate_n of birnn_layout.h, which sizes the
  // launch; spelled out here, see the note there)
  float* sh = smem;
  float* spart = sh + BC * a.HP;
  unsigned short* shb = reinterpret_cast<unsigned short*>(smem);
  float* sgate = smem + 8 * SHB;  // after 16 x SHB bf16
  float* sin = MF ? sgate + BC * MT * 16 : spart + a.KP * BC * R;  // [2][BC*J][4] step inputs (double buffer)

  // ---- weights of this workgroup in registers
  float wreg[WN];
  bf16x8 afrag[MF ? KSMAX : 1];
  const bool mv = MF ? wv < MT : tid < R * a.KP;
  const int r = tid % R, kp = tid / R;
  if constexpr (!MF) {  // thread (r, kp) holds W[row(r)][kp*KPL + i]
    const int q = r / J, u = r % J;
    const bool rv = mv && (j0 + u < H);
    const float* wrow = a.Whh + ((long long)d * GH + q * H + j0 + u) * H;
#pragma unroll
    for (int i = 0; i < WN; ++i) {
      const int k = kp * a.KPL + i;
      wreg[i] = (rv && i < a.KPL && k < H) ? wrow[k] : 0.0f;
    }
    for (int i = tid; i < BC * a.HP; i += NT) sh[i] = 0.0f;  // padding stays zero
  } else {  // lane holds A[row m*16 + (lane&15)][k = ks*32 + 8(lane>>4) + j]
    const int rl = wv * 16 + (lane & 15);
    const int q = rl / J, u = rl % J;
    const bool rv = mv && rl < R && j0 + u < H;
    const float* wrow = a.Whh + ((long long)d * GH + q * H + j0 + u) * H;
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = ks * 32 + 8 * (lane >> 4) + j;
        afrag[ks][j] = (short)bf16_rne((rv && k < H) ? wrow[k] : 0.0f);
      }
    for (int i = tid; i < 8 * SHB; i += NT) smem[i] = 0.0f;  // bf16 image incl. padding rows/cols
  }

  // ---- cell threads (waves 0-3): (b, u)
  const bool ct = tid < BC * J;
  const int cb = tid / J, cu = tid % J;
  const int cj = j0 + cu;
  const int bg = b0 + cb;
  const bool cval = ct && cj < H && bg < a.B;
  float bh[NGATE];
#pragma unroll
  for (int q = 0; q < NGATE; ++q) bh[q] = cval ? a.bhh[(long long)d * GH + q * H + cj] : 0.0f;
  float hst = 0.0f, cst = 0.0f;  // h_{t-1}, c_{t-1}

  u64* xg = a.xbuf + fwd_copies_g((long long)group * GEN_NCOPY, BC, H);  // this group's [2 slots][BC][H]
  // gather role: granule offsets and LDS destinations, fixed for the whole launch
  constexpr int GM = (BC * HM + NROLE - 1) / NROLE;
  int goff[GM], gdst[GM];
#pragma unroll
  for (int g = 0; g < GM; ++g) {
    const int i = tid - NROLE + g * NROLE;
    const bool on = tid >= NROLE && i < BC * H;
    goff[g] = on ? i : -1;
    gdst[g] = on ? (i / H) * (MF ? SHB : a.HP) + i % H : 0;
  }
  // gather role: input projection G[b][t][d][q*H + j] of every own (b, unit, gate)
  constexpr int NQ = (BC * 20 * 4 + NROLE - 1) / NROLE;
  StepLoader<NQ> ld;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = tid - NROLE + q * NROLE;  // item = gate * (BC*J) + cell
    const int gate = i / (BC * J), cell = i % (BC * J);
    const int ib = b0 + cell / J, ij = j0 + cell % J;
    const bool on = tid >= NROLE && gate < NGATE;
    ld.p[q] = (on && ib < a.B && ij < H) ? a.G + ((long long)ib * T * 2 + d) * GH + gate * H + ij : nullptr;
    ld.stride[q] = 2 * GH;
    ld.shift[q] = 0;
    ld.dst[q] = on ? cell * 4 + gate : -1;
  }
  if (tid >= NROLE) ld.issue(d == 0 ? 0 : T - 1, T);
  __syncthreads();
  STAMP_DECL

  // ---- fused-gate matvec partials: spart[kp][b][r] = sum_i W[r][kp*KPL+i] h[b][kp*KPL+i]
  auto matvec = [&]() {
    if (!mv) return;
    if constexpr (MF) {  // sgate[b][m*16 + row] = sum_k W[row][k] h[b][k]
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const unsigned short* bp = shb + (lane & 15) * SHB + 8 * (lane >> 4);
      bf16x8 bv[KSMAX];  // all B reads in flight before the MFMA chain (zero A/B beyond H)
#pragma unroll
      for (int ks = 0; ks < KSMAX; ++ks) bv[ks] = *reinterpret_cast<const bf16x8*>(bp + ks * 32);
#pragma unroll
      for (int ks = 0; ks < KSMAX; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[ks], bv[ks], acc, 0, 0, 0);
      const int col = lane & 15;
      if (col < BC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sgate[col * MT * 16 + wv * 16 + (lane >> 4) * 4 + i] = acc[i];
      }
      return;
    }
    float acc[BC];
#pragma unroll
    for (int bb = 0; bb < BC; ++bb) acc[bb] = 0.0f;
    const float* hk = sh + kp * a.KPL;
#pragma unroll
    for (int i = 0; i < WN; i += 4) {
      if (KPL_T > 0 || i < a.KPL) {
#pragma unroll
        for (int bb = 0; bb < BC; ++bb) {
          const float4 hv = *reinterpret_cast<const float4*>(hk + bb * a.HP + i);
          acc[bb] = fmaf(wreg[i], hv.x, acc[bb]);
          acc[bb] = fmaf(wreg[i + 1], hv.y, acc[bb]);
          acc[bb] = fmaf(wreg[i + 2], hv.z, acc[bb]);
          acc[bb] = fmaf(wreg[i + 3], hv.w, acc[bb]);
        }
      }
    }
#pragma unroll
    for (int bb = 0; bb < BC; ++bb) spart[(kp * BC + bb) * R + r] = acc[bb];
  };

  // Role-split loops with the same barrier sequence per step (B1, B2).  Waves 4-7
  // (gather) issue only loads, waves 0-3 (cell) only stores, so neither loop's
  // waitcnt state ever has to drain the other kind.
  if (tid >= NROLE) {
    for (int s = 0; s < T; ++s) {
      // ---- gather h_{s-1} (granules, tag s) and commit this step's inputs
      if (s > 0) {
        u64 v[GM];
        if (!gather<GM>(xg + fwd_copies_g((s - 1) & 1, BC, H), goff, (unsigned)s, v, a.spin_limit)) {
          atomicOr(a.status, 1);
          return;
        }
#pragma unroll
        for (int g = 0; g < GM; ++g)
          if (goff[g] >= 0) {
            if constexpr (MF)
              shb[gdst[g]] = bf16_rne(__uint_as_float((unsigned)v[g]));
            else
              sh[gdst[g]] = __uint_as_float((unsigned)v[g]);
          }
      }
      ld.commit(sin + (s & 1) * BC * J * 4);
      if (s + 1 < T) ld.issue(d == 0 ? s + 1 : T - 2 - s, T);
      STAMP(0)
      __syncthreads();  // B1
      STAMP(1)
      matvec();
      STAMP(2)
      __syncthreads();  // B2
      STAMP(3)
    }
    STAMP_FLUSH
    return;
  }
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? s : T - 1 - s;
    STAMP(0)
    __syncthreads();  // B1
    STAMP(1)
    matvec();
    STAMP(2)
    __syncthreads();  // B2
    STAMP(3)
    // ---- cell update for (b, u): publish first, then the saved state
    if (ct) {
      float hg[NGATE];
#pragma unroll
      for (int q = 0; q < NGATE; ++q) {
        float sacc = bh[q];
        if constexpr (MF)
          sacc += sgate[cb * MT * 16 + q * J + cu];
        else
          for (int p = 0; p < a.KP; ++p) sacc += spart[(p * BC + cb) * R + q * J + cu];
        hg[q] = sacc;
      }
      float gx[NGATE];
#pragma unroll
      for (int q = 0; q < NGATE; ++q) gx[q] = sin[(s & 1) * BC * J * 4 + tid * 4 + q];
      if (cj < H) {
        float hn = 0.0f, st[4] = {0.f, 0.f, 0.f, 0.f};
        if (cval) {
          if constexpr (CELL == CELL_LSTM) {
            const float ig = HARD ? hsig(gx[0] + hg[0]) : fsig(gx[0] + hg[0]);
            const float fg = HARD ? hsig(gx[1] + hg[1]) : fsig(gx[1] + hg[1]);
            const float gg = ftanh(gx[2] + hg[2]);
            const float og = HARD ? hsig(gx[3] + hg[3]) : fsig(gx[3] + hg[3]);
            cst = fg * cst + ig * gg;
            hn = og * ftanh(cst);
            st[0] = ig; st[1] = fg; st[2] = gg; st[3] = og;
          } else {
            const float rg = fsig(gx[0] + hg[0]);
            const float zg = fsig(gx[1] + hg[1]);
            const float ng = ftanh(gx[2] + rg * hg[2]);
            hn = (1.0f - zg) * ng + zg * hst;
            st[0] = rg; st[1] = zg; st[2] = ng; st[3] = hg[2];
          }
        }
        // padded batch rows (bg >= B) still publish (zeros) so peers never wait on them
        put_granule(xg + fwd_copies_g(s & 1, BC, H) + cb * H + cj, (unsigned)(s + 1), hn);
        if (cval) {
          const long long bt = (long long)bg * T + t;
          float* actp = a.act + (bt * 2 + d) * (4 * H) + cj;  // act rows are 4H wide for both cells
          actp[0] = st[0]; actp[H] = st[1]; actp[2 * H] = st[2]; actp[3 * H] = st[3];
          if constexpr (CELL == CELL_LSTM) a.cs[(bt * 2 + d) * H + cj] = cst;
          a.hprev[bt * 2 * H + d * H + cj] = hst;
          a.out[bt * 2 * H + d * H + cj] = hn;
        }
        hst = hn;
      }
    }
    STAMP(4)
    // sh is rewritten only after the next gather's barrier (all matvec reads are
    // behind the barrier above); spart only after that barrier too.
  }
  STAMP_FLUSH
}

namespace {
template <int CELL, int BC>
int launch_fwd_t(const RnnArgs& a, bool mf, bool hard, int grid, size_t smem, hipStream_t st) {
#ifdef RNN_EXP_MINIMAL
  return (int)hipErrorNotSupported;
#else
  if (hard) {  // Keras 1's cell: fp32 LSTM at the runtime-bounds instantiations only
    if constexpr (CELL == CELL_LSTM) {
      if (mf) return (int)hipErrorInvalidValue;
      if (a.H > HMAX) return launch_resident(rnn_fwd_kernel<CELL, BC, 0, false, HMAX_L, true>, grid, smem, st, a);
      return launch_resident(rnn_fwd_kernel<CELL, BC, 0, false, HMAX, true>, grid, smem, st, a);
    } else {
      return (int)hipErrorInvalidValue;
    }
  }
  if (a.H > HMAX) {  // forward-only large-H instantiations (the H = 600 classifier)
    if (mf)
      return launch_resident(rnn_fwd_kernel<CELL, BC, 0, true, HMAX_L>, grid, smem, st, a);
    else
      return launch_resident(rnn_fwd_kernel<CELL, BC, 0, false, HMAX_L>, grid, smem, st, a);
  }
  // compile-time k-slice lengths for the shipped H = 300 plans (LSTM J=20: 52, GRU J=20: 40)
  if (mf)
    return launch_resident(rnn_fwd_kernel<CELL, BC, 0, true>, grid, smem, st, a);
  else if (a.KPL == 52)
    return launch_resident(rnn_fwd_kernel<CELL, BC, 52, false>, grid, smem, st, a);
  else if (a.KPL == 40)
    return launch_resident(rnn_fwd_kernel<CELL, BC, 40, false>, grid, smem, st, a);
  else
    return launch_resident(rnn_fwd_kernel<CELL, BC, 0, false>, grid, smem, st, a);
#endif
}
template <int CELL>
int launch_fwd_c(const RnnArgs& a, int BC, bool mf, bool hard, int grid, size_t smem, hipStream_t st) {
  switch (BC) {
    case 1: return launch_fwd_t<CELL, 1>(a, mf, hard, grid, smem, st);
    case 2: return launch_fwd_t<CELL, 2>(a, mf, hard, grid, smem, st);
    case 4: return launch_fwd_t<CELL, 4>(a, mf, hard, grid, smem, st);
    case 8: return launch_fwd_t<CELL, 8>(a, mf, hard, grid, smem, st);
    default: return (int)hipErrorInvalidValue;
  }
}
}  // namespace

int launch_fwd(const RnnArgs& a, int cell, int BC, bool mf, bool hard, int grid, size_t smem, hipStream_t st) {
  return cell == CELL_LSTM ? launch_fwd_c<CELL_LSTM>(a, BC, mf, hard, grid, smem, st)
                           : launch_fwd_c<CELL_GRU>(a, BC, mf, hard, grid, smem, st);
}

}  // namespace dl4ss_rnn
