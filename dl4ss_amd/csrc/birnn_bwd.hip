// Generic BPTT of the persistent BiLSTM / BiGRU recurrence (one-value granules; fp32 parity mode,
// bf16 MFMA mode, the large-H instantiations) and its launch selection.  See birnn_common.h.
#include "birnn_common.h"

namespace dl4ss_rnn {

// --------------------------------------------------------------------------
// BPTT.  Step s walks time backwards for the forward direction (t = T-1-s) and
// forwards for the reverse direction.  Thread (b,u) owns dh/dc of its unit;
// the recurrent term dh_rec[b][j] = sum_{rows r} dgh[b][r] W_hh[r][j] is formed
// as per-workgroup partial sums over the workgroup's own rows (registers hold
// W[rows of w][k-group]) published for all j; each consumer gathers the NG
// partials of its own units (waves 4-7) and sums them in fixed order.
// --------------------------------------------------------------------------
//
// MF = true (bf16 MFMA mode): waves 0-3 hold W_hh^T of the workgroup's rows as bf16
// A fragments (output unit k on the MFMA row, gate row r on its K), dgh is staged
// in LDS as the bf16 B image [batch][r]; each 16-unit tile's D lanes publish their
// granules directly -- no partial-sum buffer, no third barrier.
// HM: the largest hidden size of the instantiation (sizes the per-thread offset arrays, the MFMA unit
// tiles per wave and the MFMA path's transpose area): HMAX for the mask nets, HMAX_L for the H = 600
// speaker classifier (test_multi_labels_speech.py:240-246,444).
// HARD = true: Keras 1's LSTM cell (DL4SS_RNN_HARD_GATES): the i, f and o gate derivatives are
// hard_sigmoid's, taken from the saved (clipped) activation (hsig_grad of birnn_common.h), in place of
// s (1 - s).  fp32 LSTM, runtime-bounds instantiations only.
template <int CELL, int BC, int RPL_T, int KGL_T, bool MF, int HM = HMAX, bool HARD = false>
__global__ __launch_bounds__(NT, 1) void rnn_bwd_kernel(RnnArgs a) {
  static_assert(!HARD || (CELL == CELL_LSTM && !MF && RPL_T == 0 && KGL_T == 0), "hard gates: fp32 LSTM, runtime bounds");
  constexpr int NGATE = CELL == CELL_LSTM ? 4 : 3;
  constexpr int RPLN = MF ? 1 : (RPL_T > 0 ? RPL_T : RPLMAX);  // rows per thread (compile-time)
  constexpr int KGLN = MF ? 1 : (KGL_T > 0 ? KGL_T : KGLMAX);  // k per thread (compile-time)
  constexpr int WSPAN = bwd_wspan(HM);                           // output units per MFMA wave (contiguous)
  constexpr int MTWMAX = WSPAN / 16;                             // MFMA unit tiles per wave
  constexpr int KSRMAX = (4 * JMAX + 31) / 32;                   // MFMA K-steps over gate rows (SDG: the B image's row stride)
  const int H = a.H, T = a.T, J = a.J, NG = a.NG;
  const int R = NGATE * J;
  const int ngroups = 2 * a.nchunk;
  int group, w;
  group_of(blockIdx.x, NG, ngroups, group, w);
  const int d = group / a.nchunk, chunk = group % a.nchunk;
  const int b0 = chunk * BC;
  const int j0 = w * J;
  const int tid = threadIdx.x;
  const int GH = NGATE * H;
  const int AH = 4 * H;  // act row width (LSTM i,f,g,o; GRU r,z,n and W_hn h + b_hn)
  const int RPAD = a.RP * RPLN;  // padded row count (rows >= R stay zero)
  const int KW = a.KG * KGLN;

  const int lane = tid & 63, wv = tid >> 6;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  // fp32 path: sdg [BC][RPAD] dgh of this workgroup's rows, then sdh, spart [RP][BC][KW]
  // MFMA path: sdgb bf16 [16][SDG], then sdh
  float* sdg = smem;
  unsigned short* sdgb = reinterpret_cast<unsigned short*>(smem);
  // (region lengths: bwd_sdg_n / bwd_sdh_n / bwd_spart_n of birnn_layout.h, which sizes the launch; those
  // with run-time arguments are spelled out here, see the note there)
  float* sdh = MF ? smem + 8 * SDG : sdg + BC * RPAD;  // [NG][BC][J] gathered partials
  float* spart = sdh + ((NG * BC * J + 3) & ~3);        // fp32: [RP][BC][KW]; MFMA: [4 waves][BC][WSPAN]
  float* sop = spart + (MF ? 4 * BC * WSPAN : a.RP * BC * KW);  // [2][BC*J][8] per-step operands
  for (int i = tid; i < (MF ? 8 * SDG : BC * RPAD) + NG * BC * J; i += NT) smem[i] = 0.0f;

  // fp32: thread (kg, rp): rows [rp*RPLN, +RPLN), k in [kg*KGLN, +KGLN)
  const int kg = tid % a.KG, rp = tid / a.KG;
  const bool mv = MF ? wv < 4 : rp < a.RP;
  float wreg[RPLN][KGLN];
  bf16x8 afr[MF ? MTWMAX : 1][MF ? KSRMAX : 1];
  if constexpr (!MF) {
#pragma unroll
    for (int i = 0; i < RPLN; ++i) {
      const int rr = rp * RPLN + i;
      const int q = rr / J, u = rr % J;
      const bool rv = mv && rr < R && j0 + u < H;
      const float* wrow = a.Whh + ((long long)d * GH + q * H + j0 + u) * H;
#pragma unroll
      for (int c = 0; c < KGLN; ++c) {
        const int k = kg * KGLN + c;
        wreg[i][c] = (rv && k < H) ? wrow[k] : 0.0f;
      }
    }
  } else {  // tile m = wv*MTWMAX + t: lane holds A[k = m*16 + (lane&15)][r = ks*32 + 8(lane>>4) + j] = W[row(r)][k]
#pragma unroll
    for (int t = 0; t < MTWMAX; ++t) {
      const int k = (wv * MTWMAX + t) * 16 + (lane & 15);
#pragma unroll
      for (int ks = 0; ks < KSRMAX; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int rr = ks * 32 + 8 * (lane >> 4) + j;
          const int q = rr / J, u = rr % J;
          const bool ok = mv && k < H && rr < R && j0 + u < H;
          afr[t][ks][j] = (short)bf16_rne(ok ? a.Whh[((long long)d * GH + q * H + j0 + u) * H + k] : 0.0f);
        }
    }
  }
  // gather role: offsets of the NG partials of every own (b, unit), fixed per launch
  constexpr int GM = (BC * (HM + 20) + NROLE - 1) / NROLE;
  int goff[GM];
#pragma unroll
  for (int g = 0; g < GM; ++g) {
    const int i = tid - NROLE + g * NROLE;
    goff[g] = -1;
    if (tid >= NROLE && i < NG * BC * J) {
      const int p = i / (BC * J), rem = i % (BC * J), bb = rem / J, u = rem % J;
      if (j0 + u < H) goff[g] = p * BC * H + bb * H + j0 + u;
    }
  }
  // publish role: (b, k) of every granule this thread writes, fixed per launch
  constexpr int GP = (BC * HM + NROLE - 1) / NROLE;
  int psrc[GP];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    const int i = tid + g * NROLE;
    psrc[g] = (!MF && tid < NROLE && i < BC * H) ? (i / H) * KW + i % H : -1;
  }

  const bool ct = tid < BC * J;
  const int cb = tid / J, cu = tid % J;
  const int cj = j0 + cu;
  const int bg = b0 + cb;
  const bool cval = ct && cj < H && bg < a.B;
  float dc_next = 0.0f;  // LSTM dc carried to the earlier step
  float dh_dir = 0.0f;   // GRU direct dh term carried to the earlier step

  u64* xg = a.xbuf + (long long)group * 2 * NG * BC * H;  // this group's [2 slots][NG][BC][H] (bwd_copies_g)
  // d(mean_t h) broadcast term: constant over t, loaded once by the cell thread
  const float doutb = (cval && a.dOutB) ? a.dOutB[(long long)bg * 2 * H + d * H + cj] : 0.0f;

  // gather role: per-step operands of every own (b, unit): 8 slots per cell
  //   0 dOut, 1..4 act, 5 c (LSTM) / h_prev (GRU), 6 c_prev (LSTM), 7 unused
  constexpr int NQ = (BC * 20 * 8 + NROLE - 1) / NROLE;
  StepLoader<NQ> ld;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = tid - NROLE + q * NROLE;  // item = slot * (BC*J) + cell
    const int slot = i / (BC * J), cell = i % (BC * J);
    const int ib = b0 + cell / J, ij = j0 + cell % J;
    const bool on = tid >= NROLE && slot < 8;
    const bool valid = on && ib < a.B && ij < H;
    const float* p = nullptr;
    int stride = 2 * H, shift = 0;
    if (valid) {
      if (slot == 0) {  // dOut NULL (a top layer fed by dOut_bcast alone): the item stays null and reads as zero
        if (a.dOut) p = a.dOut + (long long)ib * T * 2 * H + d * H + ij;
      } else if (slot <= 4) {
        p = a.act + ((long long)ib * T * 2 + d) * AH + (slot - 1) * H + ij;
        stride = 2 * AH;
      } else if (CELL == CELL_LSTM && (slot == 5 || slot == 6)) {
        p = a.cs + ((long long)ib * T * 2 + d) * H + ij;
        shift = slot == 6 ? (d == 0 ? -1 : 1) : 0;  // the step that ran before t in this direction
      } else if (CELL == CELL_GRU && slot == 5) {
        p = a.hprev + (long long)ib * T * 2 * H + d * H + ij;
      }
    }
    ld.p[q] = p;
    ld.stride[q] = stride;
    ld.shift[q] = shift;
    ld.dst[q] = on ? cell * 8 + slot : -1;
  }
  if (tid >= NROLE) ld.issue(d == 0 ? T - 1 : 0, T);
  STAMP_DECL

  // ---- partials P[b][k] = sum_{own rows} dgh[b][r] W[r][k]
  auto matvec = [&]() {
    if (!mv) return;
    if constexpr (MF) return;  // MFMA path: mfma_publish below
    float acc[BC][KGLN];
#pragma unroll
    for (int bb = 0; bb < BC; ++bb)
#pragma unroll
      for (int c = 0; c < KGLN; ++c) acc[bb][c] = 0.0f;
    const float* gr = sdg + rp * RPLN;
#pragma unroll
    for (int i = 0; i < RPLN; ++i) {
#pragma unroll
      for (int bb = 0; bb < BC; ++bb) {
        const float g = gr[bb * RPAD + i];  // padded rows are zero
#pragma unroll
        for (int c = 0; c < KGLN; ++c) acc[bb][c] = fmaf(g, wreg[i][c], acc[bb][c]);
      }
    }
#pragma unroll
    for (int bb = 0; bb < BC; ++bb)
#pragma unroll
      for (int c = 0; c < KGLN; ++c) spart[(rp * BC + bb) * KW + kg * KGLN + c] = acc[bb][c];
  };

  // ---- MFMA path: D[k][b] = sum_r W[r][k] dgh[b][r] per 16-unit tile, published
  //      straight from the accumulator lanes (col = batch, 4 consecutive units)
  auto mfma_publish = [&](int s) {
    const unsigned short* bp = sdgb + (lane & 15) * SDG + 8 * (lane >> 4);
    bf16x8 bv[KSRMAX];
#pragma unroll
    for (int ks = 0; ks < KSRMAX; ++ks) bv[ks] = *reinterpret_cast<const bf16x8*>(bp + ks * 32);
    // wave-private transpose: D lanes (4 consecutive units of one batch row) -> [BC][WSPAN]
    float* wsc = spart + wv * BC * WSPAN;
    const int col = lane & 15;
#pragma unroll
    for (int t = 0; t < MTWMAX; ++t) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSRMAX; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[t][ks], bv[ks], acc, 0, 0, 0);
      if (col < BC) *reinterpret_cast<f32x4*>(wsc + col * WSPAN + t * 16 + 4 * (lane >> 4)) = acc;
    }
    __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
    STAMP(4)
    // coalesced publish of this wave's contiguous unit span (granules, tag s+1)
    u64* dst = xg + (long long)(s & 1) * NG * BC * H + (long long)w * BC * H;
#pragma unroll
    for (int e0 = 0; e0 < BC * WSPAN; e0 += 64) {
      const int e = e0 + lane;
      const int bb = e / WSPAN, k = wv * WSPAN + e % WSPAN;
      if ((BC * WSPAN) % 64 == 0 || e < BC * WSPAN)
        if (k < H) put_granule(dst + bb * H + k, (unsigned)(s + 1), wsc[e]);
    }
  };

  // Role-split loops, same barrier sequence per step (B1, B2, B3 -- no B3 on the
  // MFMA path); see the forward.
  if (tid >= NROLE) {
    for (int s = 0; s < T; ++s) {
      // ---- gather the NG partials of every own unit (tag s) and commit this
      //      step's operands (issued during the previous step)
      if (s > 0) {
        u64 v[GM];
        if (!gather<GM>(xg + (long long)((s - 1) & 1) * NG * BC * H, goff, (unsigned)s, v, a.spin_limit)) {
          atomicOr(a.status, 2);
          return;
        }
#pragma unroll
        for (int g = 0; g < GM; ++g)  // sdh[i] for i = tid-256 + 256 g ; unmapped entries stay 0
          if (goff[g] >= 0) sdh[tid - NROLE + g * NROLE] = __uint_as_float((unsigned)v[g]);
      }
      ld.commit(sop + (s & 1) * BC * J * 8);
      if (s + 1 < T) ld.issue(d == 0 ? T - 2 - s : s + 1, T);
      STAMP(0)
      __syncthreads();  // B1
      STAMP(1)
      __syncthreads();  // B2
      STAMP(3)
      if (s + 1 == T) break;
      if constexpr (!MF) {
        matvec();
        STAMP(4)
        __syncthreads();  // B3
        STAMP(5)
      }
    }
    STAMP_FLUSH
    return;
  }
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? T - 1 - s : s;
    STAMP(0)
    __syncthreads();  // B1
    STAMP(1)
    // ---- cell backward for (b, u): LDS operands only, global stores only
    if (ct) {
      float dh_rec = 0.0f;
      if (s > 0) dh_rec = sum_partials(sdh + cb * J + cu, BC * J, NG);
      const float* op = sop + (s & 1) * BC * J * 8 + tid * 8;
      const float dout = op[0] + doutb;
      const float act[4] = {op[1], op[2], op[3], op[4]};
      const float c = op[5], cprev = op[6], hprev = op[5];
      float dgi[NGATE], dgh[NGATE];
      if (cval) {
        const float dh = dout + dh_rec + dh_dir;
        if constexpr (CELL == CELL_LSTM) {
          const float ig = act[0], fg = act[1], gg = act[2], og = act[3];
          const float tc = ftanh(c);
          const float dc = dc_next + dh * og * (1.0f - tc * tc);
          if constexpr (HARD) {
            dgi[0] = dc * gg * hsig_grad(ig);
            dgi[1] = dc * cprev * hsig_grad(fg);
            dgi[2] = dc * ig * (1.0f - gg * gg);
            dgi[3] = dh * tc * hsig_grad(og);
          } else {
            dgi[0] = dc * gg * ig * (1.0f - ig);
            dgi[1] = dc * cprev * fg * (1.0f - fg);
            dgi[2] = dc * ig * (1.0f - gg * gg);
            dgi[3] = dh * tc * og * (1.0f - og);
          }
          dc_next = dc * fg;
#pragma unroll
          for (int q = 0; q < NGATE; ++q) dgh[q] = dgi[q];
        } else {
          const float rg = act[0], zg = act[1], ng = act[2], hn = act[3];
          const float dn = dh * (1.0f - zg);
          const float dz = dh * (hprev - ng);
          dh_dir = dh * zg;
          const float dnp = dn * (1.0f - ng * ng);
          const float dr = dnp * hn;
          dgi[0] = dr * rg * (1.0f - rg);
          dgi[1] = dz * zg * (1.0f - zg);
          dgi[2] = dnp;
          dgh[0] = dgi[0];
          dgh[1] = dgi[1];
          dgh[2] = dnp * rg;
        }
#pragma unroll
        for (int q = 0; q < NGATE; ++q) {
          if constexpr (MF)
            sdgb[cb * SDG + q * J + cu] = bf16_rne(dgh[q]);
          else
            sdg[cb * RPAD + q * J + cu] = dgh[q];
        }
        const long long bt = (long long)bg * T + t;
        float* dgp = a.dG + (bt * 2 + d) * GH + cj;
#pragma unroll
        for (int q = 0; q < NGATE; ++q) dgp[q * H] = dgi[q];
        if (CELL == CELL_GRU) {
          float* dhp = a.dGh + (bt * 2 + d) * GH + cj;
#pragma unroll
          for (int q = 0; q < NGATE; ++q) dhp[q * H] = dgh[q];
        }
      } else {
#pragma unroll
        for (int q = 0; q < NGATE; ++q) {
          if constexpr (MF)
            sdgb[cb * SDG + q * J + cu] = 0;
          else
            sdg[cb * RPAD + q * J + cu] = 0.0f;
        }
      }
    }
    STAMP(2)
    __syncthreads();  // B2
    STAMP(3)
    if (s + 1 == T) break;  // nothing flows past the sequence start
    if constexpr (MF) {
      mfma_publish(s);
      STAMP(6)
      continue;
    }
    matvec();
    STAMP(4)
    __syncthreads();  // B3
    STAMP(5)
    // ---- reduce over row parts and publish granules (tag s+1): waves 0-3 only
    {
      u64* dst = xg + (long long)(s & 1) * NG * BC * H + (long long)w * BC * H;
#pragma unroll
      for (int g = 0; g < GP; ++g) {
        if (psrc[g] >= 0) {
          float v = 0.0f;
          for (int p = 0; p < a.RP; ++p) v += spart[p * BC * KW + psrc[g]];
          put_granule(dst + tid + g * NROLE, (unsigned)(s + 1), v);
        }
      }
    }
    STAMP(6)
    // sdg is rewritten after the next gather barrier, spart after the next cell
    // barrier, sdh after this step's barriers: every reader is behind them.
  }
  STAMP_FLUSH
}

namespace {
template <int CELL, int BC>
int launch_bwd_t(const RnnArgs& a, bool mf, bool hard, int grid, size_t smem, hipStream_t st) {
#ifdef RNN_EXP_MINIMAL
  return (int)hipErrorNotSupported;
#else
  if (hard) {  // Keras 1's cell: fp32 LSTM at the runtime-bounds instantiations only (the caller sized smem for them)
    if constexpr (CELL == CELL_LSTM) {
      if (mf) return (int)hipErrorInvalidValue;
      if (a.H > HMAX) return launch_resident(rnn_bwd_kernel<CELL, BC, 0, 0, false, HMAX_L, true>, grid, smem, st, a);
      return launch_resident(rnn_bwd_kernel<CELL, BC, 0, 0, false, HMAX, true>, grid, smem, st, a);
    } else {
      return (int)hipErrorInvalidValue;
    }
  }
  int rpln, kgln;
  bwd_dims(a.RPL, a.KGL, rpln, kgln, a.H > HMAX);
  if (a.H > HMAX) {  // large-H instantiations (the H = 600 classifier)
    if (mf) return launch_resident(rnn_bwd_kernel<CELL, BC, 0, 0, true, HMAX_L>, grid, smem, st, a);
    if (rpln == 16 && kgln == 4) return launch_resident(rnn_bwd_kernel<CELL, BC, 16, 4, false, HMAX_L>, grid, smem, st, a);
    return launch_resident(rnn_bwd_kernel<CELL, BC, 0, 0, false, HMAX_L>, grid, smem, st, a);
  }
  if (mf)
    return launch_resident(rnn_bwd_kernel<CELL, BC, 0, 0, true>, grid, smem, st, a);
  else if (rpln == 20 && kgln == 3)
    return launch_resident(rnn_bwd_kernel<CELL, BC, 20, 3, false>, grid, smem, st, a);
  else if (rpln == 20 && kgln == 2)
    return launch_resident(rnn_bwd_kernel<CELL, BC, 20, 2, false>, grid, smem, st, a);
  else
    return launch_resident(rnn_bwd_kernel<CELL, BC, 0, 0, false>, grid, smem, st, a);
#endif
}
template <int CELL>
int launch_bwd_c(const RnnArgs& a, int BC, bool mf, bool hard, int grid, size_t smem, hipStream_t st) {
  switch (BC) {
    case 1: return launch_bwd_t<CELL, 1>(a, mf, hard, grid, smem, st);
    case 2: return launch_bwd_t<CELL, 2>(a, mf, hard, grid, smem, st);
    case 4: return launch_bwd_t<CELL, 4>(a, mf, hard, grid, smem, st);
    case 8: return launch_bwd_t<CELL, 8>(a, mf, hard, grid, smem, st);
    default: return (int)hipErrorInvalidValue;
  }
}
}  // namespace

int launch_bwd(const RnnArgs& a, int cell, int BC, bool mf, bool hard, int grid, size_t smem, hipStream_t st) {
  return cell == CELL_LSTM ? launch_bwd_c<CELL_LSTM>(a, BC, mf, hard, grid, smem, st)
                           : launch_bwd_c<CELL_GRU>(a, BC, mf, hard, grid, smem, st);
}

}  // namespace dl4ss_rnn
