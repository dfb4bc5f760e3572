// Packed BPTT of the persistent BiLSTM / BiGRU recurrence (bf16 MFMA mode, packed hand-off: the
// training step's backward) and its launch selection.  See birnn_common.h.
#include "birnn_common.h"

namespace dl4ss_rnn {

// --------------------------------------------------------------------------
// BPTT, bf16 MFMA mode with the packed hand-off (the throughput path; see the
// packed forward, birnn_fwd_pk.hip, for the measurements behind each choice).  What crosses
// workgroups per step are the partial sums P_w[b][k] = sum_{own rows r} dgh[b][r]
// W[r][k]; they are packed as 24-bit floats (fp32 rounded to 15 mantissa bits,
// relative error <= 2^-16, far below the bf16 rounding of dgh itself), two per
// tagged 8-B granule:
//   granule = { lo: p0 | (p1 & 0xFF) << 24, hi: (p1 >> 8) | tag << 16 }
// one 16-B store per 4 units (two granules), plain or `sc1` by the group's placement,
// buffer [slot][copy][producer][b][HG granules], HG = H/2 rounded up to even.
// Waves: 0-3 cell backward (rows b = tid/32) + MFMA W^T dgh + publish;
//        4 polls the NG producers' partials of the own J units into LDS;
//        5-7 per-step operand prefetch.
// --------------------------------------------------------------------------
// The prefetch waves' per-step operand loads share the consumer CU's memory queue with the polls, and
// their price is paid in the hand-off (round 6: BPTT 331 -> 289 us per launch without them, results
// wrong); non-temporal operand loads were slower (376 us), the last forward layer's act / c saved
// with plain stores for the top BPTT no faster.
// The cell lanes' dG / dGh stores of step s-1 issued after B1 of step s (before the cell update)
// instead of right after the publish: measured slower, 7994 vs 8085 mixtures/s
// (profiles/r03_dglate.jsonl) -- their issue then sits on the cell phase's critical path
__device__ __forceinline__ unsigned pack24(float v) {
  const unsigned u = __float_as_uint(v);
  return (u + 0x80u) >> 8;  // round to nearest (ties away) on the dropped 8 bits
}
__device__ __forceinline__ float unpack24(unsigned r) { return __uint_as_float(r << 8); }

template <int CELL, int BC, int NZ = 1>
__global__ __launch_bounds__(NT, 1) void rnn_bwd_pk_kernel(RnnArgs a) {
  constexpr int NGATE = CELL == CELL_LSTM ? 4 : 3;
  // partial-sum slots of the gather (polling waves): a lane group of BSL_Q lanes = every (b, quad)
  // of one slot at J <= 20; BSL_G groups per polling wave; BSL_N slots; GLK producers per lane
  constexpr int BSL_Q = BC * 5;
  constexpr int BSL_G = 64 / BSL_Q > 0 ? 64 / BSL_Q : 1;
  constexpr int BSL_N = BWD_NPW * BSL_G < 16 ? BWD_NPW * BSL_G : 16;
  constexpr int GLK = (16 + BSL_N - 1) / BSL_N;  // NG <= 16
  static_assert(BSL_Q <= 64, "one (b, quad) item per lane");
  constexpr int WSPAN = bwd_wspan(HMAX);       // output units per MFMA wave (80)
  constexpr int MTWMAX = WSPAN / 16;           // MFMA unit tiles per wave (5)
  constexpr int KSRMAX = (4 * JMAX + 31) / 32; // MFMA K-steps over gate rows (3; SDG: the dgh B image's row stride)
  constexpr int WSP = BWD_PK_WSP;              // transpose row stride (floats): rows on distinct bank quads
  const int H = a.H, T = a.T, J = a.J, NG = a.NG;
  const int R = NGATE * J;
  const int ngroups = 2 * a.nchunk;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int group, w;
  group_pk(a.gctl, NG, ngroups, a.spin_limit, a.status, smem, group, w);
  const int d = group / a.nchunk, chunk = group % a.nchunk;
  const int b0 = chunk * BC;
  const int j0 = w * J;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int GH = NGATE * H;
  const int AH = 4 * H;
  const int HG = ((H + 1) / 2 + 1) & ~1;  // pk_hg: granules per (producer, row), even: 16-B aligned rows

  unsigned short* sdgb = reinterpret_cast<unsigned short*>(smem);  // [16][SDG] bf16 dgh B image
  float* sdh = smem + 8 * SDG;                                      // [16][BC][J] gathered partials (rows >= NG stay 0)
  float* wsc = sdh + ((16 * BC * J + 3) & ~3);                      // [4 waves][BC][WSP] (bwd_pk_sdh_n)
  // per-step operands, [2 steps][2 planes][cell = b * J + u][4] (slots 0-3 in plane 0, 4-7 in
  // plane 1): the cell lanes read their two 16-B quads conflict-free (16 lanes on 16 consecutive
  // cells), and so is the prefetch commit (below)
  constexpr int SOPP = bwd_pk_sopp(BC);
  constexpr int WSCN = bwd_pk_wsc_n(BC), SOPN = bwd_pk_sop_n(BC);  // (constexpr variables: see birnn_layout.h)
  float* sop = wsc + WSCN;
  for (int i = tid; i < 8 * SDG + 16 * BC * J; i += NT) smem[i] = 0.0f;

  // ---- W_hh^T tiles (waves 0-3): tile m = wv*MTWMAX + t, lane holds
  //      A[k = m*16 + (lane&15)][r = ks*32 + 8(lane>>4) + j] = W[row(r)][k]
  const bool mv = wv < 4;
  bf16x8 afr[MTWMAX][KSRMAX];
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

  // ---- cell lanes: row cb = tid / 32, unit cu = tid % 32 (< J)
  const int cb = tid >> 5, cu = tid & 31;
  const bool ct = tid < BC * 32 && cu < J;
  const int cj = j0 + cu;
  const int bg = b0 + cb;
  const bool cval = ct && cj < H && bg < a.B;
  float dc_next = 0.0f, dh_dir = 0.0f;
  const float doutb = (cval && a.dOutB) ? a.dOutB[(long long)bg * 2 * H + d * H + cj] : 0.0f;

  // partial-sum granules of this group: [2 slots][hand-off, spare][NG][BC][HG] x 8 B; the
  // spare copy of slot 1 holds the placement granules
  const int copy_g = NG * BC * HG;  // bwd_pk_copy_g
  u64* xg = a.xbuf + (long long)group * PK_NCOPY * copy_g;
  const __amdgpu_buffer_rsrc_t xr = granule_rsrc(xg, (unsigned)(PK_NCOPY * copy_g * 8));
  __shared__ int s_wt;
  if (tid == 0) __hip_atomic_store(xg + PK_PLACE_COPY * copy_g + w, (1ull << 32) | xcc_id(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (wv == WPOLL) {
    const bool wt = group_needs_write_through(xg + PK_PLACE_COPY * copy_g, NG, lane, a.spin_limit, a.status, a.place_force);
    if (lane == 0) s_wt = wt;
  }

  // ---- prefetch waves WPF..7: per-step operands of every own (b, unit): 8 slots per cell
  //   0 dOut, 1..4 act, 5 c (LSTM) / h_prev (GRU), 6 c_prev (LSTM), 7 unused
  constexpr int WPF = WPOLL + BWD_NPW;  // waves WPOLL .. WPF-1 poll
  constexpr int NPF = NT - WPF * 64;
  // (round 3 committed the raw operands straight into the cell lanes' record, slot-major: 16-B
  // strided words, a 4-way conflict -- SQ_LDS_BANK_CONFLICT / IDX_ACTIVE 0.036 -> 0.157; cell-major
  // items were conflict-free but touched one cache line per lane octet and held the prefetch waves
  // ~650 cycles past the cell phase, profiles/r03_pfmap_stamps.txt)
  constexpr int NSL = CELL == CELL_LSTM ? 7 : 6;
  // each prefetch wave owns half of the cells (cpw of them) and stages their raw operands
  // slot-major in a wave-private LDS block [NSL][CPWP] (a load instruction's lanes read consecutive
  // units of one operand row; consecutive lanes commit consecutive words), then one lane per cell
  // turns them into the cell's step factors (pf_factors)
  // (BC >= 4 only.  At BC <= 2 the raw operands go straight into the record as slot-major items --
  // 64 consecutive cells of one slot per load instruction, a 4-way commit conflict: there the
  // step is short and the loads' spread decides; 4 slots x 8 cells per half-wave (conflict-free,
  // twice the cache lines per instruction) took the BiGRU C3 BPTT from 325 to 407 us per launch)
  static_assert(NPF == 128, "two prefetch waves");
  constexpr bool PFF = BC >= 4;
  constexpr int CPWP = bwd_pk_cpwp(BC);  // raw staging pitch: cells per prefetch wave at J <= 20
  // PFF: the act slots 1-4 arrive as ONE 16-B item per cell (the cell-major act of the packed
  // forward, a.act_cm, required at BC >= 4 by the launcher); the scalar loader carries dOut and
  // (LSTM) c_prev = c at the step's neighbour t -+ 1, or (GRU) h_prev.  The LSTM's c of a step is
  // the c_prev the previous step loaded: pf_factors keeps it in the slot-5 row for the next step
  // (one scalar load per cell and step fewer; the first step's c is loaded once before the loop)
  constexpr int NSLS = 2;
  constexpr int NQ = PFF ? (NSLS * CPWP + 63) / 64 : (BC * 20 * NSL + NPF - 1) / NPF;
  constexpr int NQA = PFF ? (CPWP + 63) / 64 : 1;
  const int ncell = BC * J, cpw = (ncell + 1) / 2, pwi = wv - WPF;
  float* sraw = sop + SOPN +(wv >= WPF ? pwi : 0) * NSL * CPWP;
  StepLoader<NQ, NZ> ld;  // dOut: NZ split-K slabs (DL4SS_RNN_DOUT_SLABS)
  ld.zs = a.dout_zs;
  const float4* ap[NQA];
  float4 av[NQA];
  // At batch chunks >= 4 (the step-factor prefetch) two steps' operand loads are in flight, ld2 / av2
  // the odd steps' operands.  At BC <= 2 (raw operands straight into the record) one step ahead stays:
  // C1's B = 1 step measured 461 vs 468 mixtures/s with two (profiles/r06_cfg_pf2.txt)
  StepLoader<NQ, NZ> ld2;
  float4 av2[NQA];
  int ac[NQA];
#pragma unroll
  for (int q = 0; q < NQA; ++q) {
    const int c = lane + 64 * q, cell = pwi * cpw + c;
    const int ib = b0 + cell / J, ij = j0 + cell % J;
    const bool ok = PFF && wv >= WPF && c < cpw && cell < ncell;
    ap[q] = (ok && ib < a.B && ij < H) ? reinterpret_cast<const float4*>(a.act) + ((long long)ib * T * 2 + d) * H + ij
                                       : nullptr;
    ac[q] = ok ? c : -1;
    av[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  auto act_issue = [&](float4* v, int t) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < NQA; ++q)
      v[q] = ap[q] != nullptr ? ap[q][(long long)t * 2 * H] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto act_commit = [&](const float4* v) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < NQA; ++q)
      if (ac[q] >= 0) {
        sraw[1 * CPWP + ac[q]] = v[q].x;
        sraw[2 * CPWP + ac[q]] = v[q].y;
        sraw[3 * CPWP + ac[q]] = v[q].z;
        sraw[4 * CPWP + ac[q]] = v[q].w;
      }
  };
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    int slot, c = 0, cell;
    bool on;
    if constexpr (PFF) {
      const int i = lane + 64 * q;
      const int ss = i / cpw;  // scalar slot 0, 1 -> slot 0, and 6 (LSTM c_prev) / 5 (GRU h_prev)
      slot = ss == 0 ? 0 : CELL == CELL_LSTM ? 6 : 5;
      c = i - ss * cpw;
      cell = pwi * cpw + c;
      on = wv >= WPF && ss < NSLS && cell < ncell;
    } else {
      const int i = tid - WPF * 64 + q * NPF;
      slot = i / ncell;
      cell = i - slot * ncell;
      on = wv >= WPF && i >= 0 && slot < NSL;
    }
    const int ib = b0 + cell / J, iu = cell % J, ij = j0 + iu;
    const bool valid = on && ib < a.B && ij < H;
    const float* p = nullptr;
    int stride = 2 * H, shift = 0;
    if (valid) {
      if (slot == 0) {
        p = a.dOut + (long long)ib * T * 2 * H + d * H + ij;
      } else if (slot <= 4) {
        p = a.act + ((long long)ib * T * 2 + d) * AH + (slot - 1) * H + ij;
        stride = 2 * AH;
      } else if (CELL == CELL_LSTM && (slot == 5 || slot == 6)) {
        p = a.cs + ((long long)ib * T * 2 + d) * H + ij;
        shift = slot == 6 ? (d == 0 ? -1 : 1) : 0;
      } else if (CELL == CELL_GRU && slot == 5) {
        p = a.hprev + (long long)ib * T * 2 * H + d * H + ij;
      }
    }
    ld.p[q] = p;
    ld.stride[q] = stride;
    ld.shift[q] = shift;
    ld.dst[q] = !on ? -1 : PFF ? slot * CPWP + c : (slot >> 2) * SOPP + cell * 4 + (slot & 3);
    ld.zq[q] = slot == 0;
  }
  auto tstep = [&](int s) { return d == 0 ? T - 1 - s : s; };  // time index of BPTT step s
  if constexpr (PFF) ld2 = ld;
  if (wv >= WPF) {
    ld.issue(tstep(0), T);
    if constexpr (PFF) act_issue(av, tstep(0));
    if (PFF && T > 1) {
      ld2.issue(tstep(1), T);
      if constexpr (PFF) act_issue(av2, tstep(1));
    }
    if constexpr (PFF && CELL == CELL_LSTM) {  // the first step's c (later steps reuse c_prev)
      const int t0 = d == 0 ? T - 1 : 0;
      for (int c = lane; c < cpw; c += 64) {
        const int cell = pwi * cpw + c;
        const int ib = b0 + cell / J, ij = j0 + cell % J;
        sraw[5 * CPWP + c] = (cell < ncell && ib < a.B && ij < H) ? a.cs[((long long)(ib * T + t0) * 2 + d) * H + ij]
                                                                     : 0.0f;
      }
    }
  }
  __syncthreads();
  const bool wt = __builtin_amdgcn_readfirstlane(s_wt) != 0;  // granules written through (group spans XCDs)
  if (tid == 0) release_start(a.gctl, a.xbuf, ngroups, NG, (long long)PK_NCOPY * copy_g, (long long)PK_PLACE_COPY * copy_g);
  STAMP_DECL

  if (wv >= WPOLL && wv < WPF) {
    // ---- polling waves: a lane owns one (b, quad of 4 units) and BSL_P producers of it -- slot
    //      sl = pw * BSL_G + (lane / (5 BC)), producers sl, sl + BSL_N, ... -- and sums their
    //      partials in registers: the cell lanes then add BSL_N slot partials instead of NG
    //      producer partials (16 LDS reads + a 16-leaf tree cost ~150 cycles of the cell phase,
    //      round-4 stamps).  Lanes of a group read consecutive quads of one producer row (the
    //      sweep touches as many cache lines as a producer-major map).
    const int pw = wv - WPOLL;
    const int JQ = J / 4;
    const int gi = lane / BSL_Q, bq = lane % BSL_Q;
    const int pb_b = bq / 5, qd = bq % 5;
    const int sl = pw * BSL_G + gi;
    const bool lane_on = gi < BSL_G && sl < BSL_N && qd < JQ && pb_b < BC;
    int loff[GLK];
    bool on[GLK];
#pragma unroll
    for (int g = 0; g < GLK; ++g) {
      const int p = sl + BSL_N * g;
      on[g] = lane_on && p < NG;
      loff[g] = on[g] ? (p * BC + pb_b) * HG + (j0 >> 1) + 2 * qd : 0;  // granule offset within a copy
    }
    const int doff = lane_on ? (sl * BC + pb_b) * J + 4 * qd : 0;  // sdh[(slot * BC + b) * J + u]
    for (int s = 0; s < T; ++s) {
      if (s > 0) {
        const unsigned tag = (unsigned)s & 0xFFFFu;
        if (wv == WPOLL) TRACE(2, s);
        // 16-B `sc1` buffer loads, one per granule pair (half the requests of the 8-B atomic
        // loads: BPTT 4800 -> 4153, forward 3302 -> 3111 cycles per step); the empty asm with a
        // memory clobber keeps every sweep inside the loop (the buffer intrinsic is a plain
        // read-only load to the compiler: hoisted out of the spin loop without it)
        const int sb = ((s - 1) & 1) * 2 * copy_g * 8;  // the slot's hand-off copy (bytes)
        u32x4 q[GLK], qa[GLK], qb[GLK];
        unsigned done = 0;
        asm volatile("" ::: "memory");
#pragma unroll
        for (int g = 0; g < GLK; ++g) qa[g] = __builtin_amdgcn_raw_buffer_load_b128(xr, sb + loff[g] * 8, 0, 16);
        unsigned spins = 0;
        while (true) {
          asm volatile("" ::: "memory");
#pragma unroll
          for (int g = 0; g < GLK; ++g) qb[g] = __builtin_amdgcn_raw_buffer_load_b128(xr, sb + loff[g] * 8, 0, 16);
#pragma unroll
          for (int g = 0; g < GLK; ++g) {
            const bool m = ((qa[g].y >> 16) == tag) & ((qa[g].w >> 16) == tag) & !((done >> g) & 1);
            q[g] = m ? qa[g] : q[g];
            done |= (unsigned)m << g;
          }
          if (done == (1u << GLK) - 1) break;
          asm volatile("" ::: "memory");
#pragma unroll
          for (int g = 0; g < GLK; ++g) qa[g] = __builtin_amdgcn_raw_buffer_load_b128(xr, sb + loff[g] * 8, 0, 16);
#pragma unroll
          for (int g = 0; g < GLK; ++g) {
            const bool m = ((qb[g].y >> 16) == tag) & ((qb[g].w >> 16) == tag) & !((done >> g) & 1);
            q[g] = m ? qb[g] : q[g];
            done |= (unsigned)m << g;
          }
          if (done == (1u << GLK) - 1) break;
          if (++spins > a.spin_limit) {
            atomicOr(a.status, 2);
            return;
          }
        }
        float4 acc4 = make_float4(0.f, 0.f, 0.f, 0.f);  // this lane's producers, summed in order g
#pragma unroll
        for (int g = 0; g < GLK; ++g) {
          if (on[g]) {
            const unsigned l0 = q[g].x, l1 = q[g].y, h0 = q[g].z, h1 = q[g].w;
            acc4.x += unpack24(l0 & 0xFFFFFFu);
            acc4.y += unpack24((l0 >> 24) | ((l1 & 0xFFFFu) << 8));
            acc4.z += unpack24(h0 & 0xFFFFFFu);
            acc4.w += unpack24((h0 >> 24) | ((h1 & 0xFFFFu) << 8));
          }
        }
        if (lane_on) *reinterpret_cast<float4*>(sdh + doff) = acc4;  // 16-B aligned: J % 4 == 0
        if (wv == WPOLL) TRACE(1, s);
      }
      STAMP(0)
      __syncthreads();  // B1
      STAMP(1)
      __syncthreads();  // B2
      STAMP(3)
      if (s + 1 == T) break;
    }
    STAMP_FLUSH
    return;
  }
  if (wv >= WPF) {
    // the step factors of this wave's cells: everything of the cell backward that does not depend
    // on the gathered dh, off the cell lanes' B1 -> B2 path (LSTM: tanh(c) and the gate
    // derivatives; GRU: the z / n / r products), into the record the cell lanes read after B1:
    //   LSTM {dOut, o (1 - tanh^2 c), g i (1 - i), c_prev f (1 - f)} {i (1 - g^2), tanh(c) o (1 - o), f, -}
    //   GRU  {dOut, (1-z)(1-n^2) hn r (1-r), (h_prev - n) z (1-z), (1-z)(1-n^2)} {(1-z)(1-n^2) r, z, -, -}
    auto pf_factors = [&](int s, const StepLoader<NQ, NZ>& L, const float4* A) __attribute__((always_inline)) {
      L.commit(sraw);
      act_commit(A);
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
      // one lane per cell, in passes of 64: cpw = ceil(BC J / 2) is 80 at BC = 8, J = 20
      for (int c = lane; c < cpw; c += 64) {
        const int cell = pwi * cpw + c;
        if (cell >= ncell) break;
        float v[NSL];
#pragma unroll
        for (int k = 0; k < NSL; ++k) v[k] = sraw[k * CPWP + c];
        float4 p0, p1;
        if constexpr (CELL == CELL_LSTM) {
          const float ig = v[1], fg = v[2], gg = v[3], og = v[4];
          const float tc = ftanh(v[5]);
          p0 = make_float4(v[0], og * (1.0f - tc * tc), gg * ig * (1.0f - ig), v[6] * fg * (1.0f - fg));
          p1 = make_float4(ig * (1.0f - gg * gg), tc * og * (1.0f - og), fg, 0.0f);
        } else {
          const float rg = v[1], zg = v[2], ng = v[3], hn = v[4];
          const float gn = (1.0f - zg) * (1.0f - ng * ng);
          p0 = make_float4(v[0], gn * hn * rg * (1.0f - rg), (v[5] - ng) * zg * (1.0f - zg), gn);
          p1 = make_float4(gn * rg, zg, 0.0f, 0.0f);
        }
        float* rec = sop + (s & 1) * 2 * SOPP + cell * 4;
        *reinterpret_cast<float4*>(rec) = p0;
        *reinterpret_cast<float4*>(rec + SOPP) = p1;
        if constexpr (CELL == CELL_LSTM) sraw[5 * CPWP + c] = v[6];  // the next step's c
      }
    };
    // Either way the loads go out after B1, in the cell phase: not in the CU's memory queue beside the
    // polling sweeps (MI355X_MICROARCH.md handoff-1to1: the hand-off price sits in the consumer CU's
    // queue); they still have the cell phase and the next poll window to land
    if constexpr (PFF) {
      // two steps in flight: step s's operands were issued in step s - 2 (ld for even s, ld2 for odd), so
      // a load has a whole step more than the cell phase + hand-off window to land before the commit
      // (round 6: with one step ahead the commit waited on them -- two more dOut loads per cell for the
      // split-K slabs cost ~8 us per launch, profiles/r06_nz_ab.txt).
      // The even / odd pair is straight-line code, the loads issued every step (past the end the last
      // step's again, unused): the same loads in flight at every commit, so hipcc's waitcnt pass keeps
      // the newer step's loads in flight at each commit -- BPTT 331 -> 322 us per launch against an
      // even / odd branch, bitwise (profiles/r06_pf2_unroll_ab.txt)
      auto pf_step = [&](int s, StepLoader<NQ, NZ>& L, float4* A) __attribute__((always_inline)) {
        pf_factors(s, L, A);
        __syncthreads();  // B1
        const int tn = tstep(min(s + 2, T - 1));
        L.issue(tn, T);
        act_issue(A, tn);
        __syncthreads();  // B2
      };
      int s = 0;
      for (; s + 1 < T; s += 2) {
        pf_step(s, ld, av);
        pf_step(s + 1, ld2, av2);
      }
      if (s < T) pf_step(s, ld, av);
    } else {
      for (int s = 0; s < T; ++s) {
        ld.commit(sop + (s & 1) * 2 * SOPP);
        __syncthreads();  // B1
        if (s + 1 < T) ld.issue(tstep(s + 1), T);
        __syncthreads();  // B2
        if (s + 1 == T) break;
      }
    }
    return;
  }

  // ---- waves 0-3: cell backward, then MFMA partials and their publish
  float sbi[NGATE], sbh[NGATE];  // this cell's bias-gradient sums over t
  float pgi[NGATE], pgh[NGATE];  // this step's dG / dGh, stored after the publish
  int pt = 0;
#pragma unroll
  for (int q = 0; q < NGATE; ++q) sbi[q] = sbh[q] = pgi[q] = pgh[q] = 0.0f;
  auto store_dg = [&]() {
    if (!cval) return;
    const long long go = (long long)((bg * T + pt) * 2 + d) * GH + cj;
    if (a.dG) {
#pragma unroll
      for (int q = 0; q < NGATE; ++q) a.dG[go + q * H] = pgi[q];
    }
    if (a.dGb) {
#pragma unroll
      for (int q = 0; q < NGATE; ++q) a.dGb[go + q * H] = bf16_rne(pgi[q]);
    }
    if (CELL == CELL_GRU) {
      if (a.dGh) {
#pragma unroll
        for (int q = 0; q < NGATE; ++q) a.dGh[go + q * H] = pgh[q];
      }
      if (a.dGhb) {
        const long long goh = (long long)((bg * T + pt) * 2 + d) * a.ghb + cj;
#pragma unroll
        for (int q = 0; q < NGATE; ++q) a.dGhb[goh + q * H] = bf16_rne(pgh[q]);
      }
    }
  };
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? T - 1 - s : s;
    STAMP(0)
    __syncthreads();  // B1
    STAMP(1)
    if (tid == 0) TRACE(3, s);
    if (tid < BC * 32) {
      float dgi[NGATE], dgh[NGATE];
#pragma unroll
      for (int q = 0; q < NGATE; ++q) dgi[q] = dgh[q] = 0.0f;
      if (cval) {
        // two 16-B reads per lane (the record's two planes), issued first, with the slot
        // partial reads behind them in the same LDS round trip (sdh is zero before the first gather)
        const int rec = (s & 1) * 2 * SOPP + (cb * J + cu) * 4;
        const float4 o0 = *reinterpret_cast<const float4*>(sop + rec);
        const float4 o1 = *reinterpret_cast<const float4*>(sop + rec + SOPP);
        const float dh_rec = sum_slots<BSL_N>(sdh + cb * J + cu, BC * J);
        const float dout = o0.x + doutb;
        const float dh = dout + dh_rec + dh_dir;
        STAMP(7)
        if constexpr (PFF && CELL == CELL_LSTM) {  // the record holds the step factors (pf_factors)
          const float dc = dc_next + dh * o0.y;
          dgi[0] = dc * o0.z;
          dgi[1] = dc * o0.w;
          dgi[2] = dc * o1.x;
          dgi[3] = dh * o1.y;
          dc_next = dc * o1.z;
#pragma unroll
          for (int q = 0; q < NGATE; ++q) dgh[q] = dgi[q];
        } else if constexpr (PFF) {
          dgi[0] = dh * o0.y;
          dgi[1] = dh * o0.z;
          dgi[2] = dh * o0.w;
          dgh[0] = dgi[0];
          dgh[1] = dgi[1];
          dgh[2] = dh * o1.x;
          dh_dir = dh * o1.y;
        } else if constexpr (CELL == CELL_LSTM) {  // raw operands {dOut, i, f, g} {o, c, c_prev, -}
          const float ig = o0.y, fg = o0.z, gg = o0.w, og = o1.x;
          const float tc = ftanh(o1.y);
          const float dc = dc_next + dh * og * (1.0f - tc * tc);
          dgi[0] = dc * gg * ig * (1.0f - ig);
          dgi[1] = dc * o1.z * fg * (1.0f - fg);
          dgi[2] = dc * ig * (1.0f - gg * gg);
          dgi[3] = dh * tc * og * (1.0f - og);
          dc_next = dc * fg;
#pragma unroll
          for (int q = 0; q < NGATE; ++q) dgh[q] = dgi[q];
        } else {  // raw operands {dOut, r, z, n} {hn, h_prev, -, -}
          const float rg = o0.y, zg = o0.z, ng = o0.w, hn = o1.x;
          const float dn = dh * (1.0f - zg);
          const float dz = dh * (o1.y - ng);
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
          sbi[q] += dgi[q];
          sbh[q] += dgh[q];
          pgi[q] = dgi[q];
          pgh[q] = dgh[q];
        }
      }
      if (ct) {
#pragma unroll
        for (int q = 0; q < NGATE; ++q) sdgb[cb * SDG + q * J + cu] = bf16_rne(dgh[q]);
      }
    }
    pt = t;
    STAMP(2)
    __syncthreads();  // B2
    STAMP(3)
    if (s + 1 == T) {  // nothing flows past the sequence start
      store_dg();
      break;
    }
    // ---- D[k][b] = sum_r W[r][k] dgh[b][r] per 16-unit tile, packed four units per 16-B store: at BC = 4
    //      and below the quads are spread over the wave by DPP row shifts (round 6: bitwise the LDS-transposed
    //      form, -35 us per C2 step, profiles/r06_bwd_pub_dpp_ab.txt), at BC = 8 transposed through
    //      wave-private LDS to [b][unit].  (Round 4's register-direct form -- five 16-lane stores per wave --
    //      lost to the transpose; the DPP form keeps the transpose's two full stores and drops its LDS trip.)
    {
      // rows >= BC of the dgh B image are zero: read row BC (broadcast, conflict-free B reads)
      const unsigned short* bp = sdgb + min(lane & 15, BC) * SDG + 8 * (lane >> 4);
      bf16x8 bv[KSRMAX];
#pragma unroll
      for (int ks = 0; ks < KSRMAX; ++ks) bv[ks] = *reinterpret_cast<const bf16x8*>(bp + ks * 32);
      float* wsw = wsc + wv * BC * WSP;
      const int col = lane & 15;
      // k-step-major over the wave's tiles: MTWMAX independent chains in flight
      f32x4 acc[MTWMAX];
#pragma unroll
      for (int t2 = 0; t2 < MTWMAX; ++t2) acc[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSRMAX; ++ks)
#pragma unroll
        for (int t2 = 0; t2 < MTWMAX; ++t2)
          acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[t2][ks], bv[ks], acc[t2], 0, 0, 0);
      if constexpr (BC == 4 && MTWMAX == 5) {
        // lane 16 g + b (b < 4) holds tile t's four units 16 t + 4 g .. + 3 of batch row b.  Tiles 0-3 go out
        // in ONE full-wave 16-B store: lane 16 g + 4 t + b takes tile t's quad from lane 16 g + b by a DPP row
        // shift of 4 t into bank t (no LDS transpose); tile 4 from its own 16 lanes
        const unsigned tag = (unsigned)(s + 1) & 0xFFFFu;
        f32x4 xq = acc[0];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          int v = __float_as_int(xq[c]);
          v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[1][c]), 0x114, 0xF, 0x2, false);  // row_shr:4
          v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[2][c]), 0x118, 0xF, 0x4, false);  // row_shr:8
          v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[3][c]), 0x11C, 0xF, 0x8, false);  // row_shr:12
          xq[c] = __int_as_float(v);
        }
        const int bb = lane & 3, g = lane >> 4;
        auto put = [&](const f32x4 v, int k) __attribute__((always_inline)) {
          const unsigned r0 = pack24(v[0]), r1 = pack24(v[1]), r2 = pack24(v[2]), r3 = pack24(v[3]);
          const u32x4 x = {r0 | (r1 << 24), (r1 >> 8) | (tag << 16), r2 | (r3 << 24), (r3 >> 8) | (tag << 16)};
          const int off = (((s & 1) * 2 * NG + w) * BC + bb) * HG + (k >> 1);  // granules
          if (wt)
            __builtin_amdgcn_raw_buffer_store_b128(x, xr, off * 8, 0, 16);  // sc1 write-through (group spans XCDs)
          else
            __builtin_amdgcn_raw_buffer_store_b128(x, xr, off * 8, 0, 0);   // plain: stays in the group's L2
        };
        const int k0 = wv * WSPAN + 16 * ((lane >> 2) & 3) + 4 * g;
        if (k0 < H) put(xq, k0);
        const int k4 = wv * WSPAN + 64 + 4 * g;
        if ((lane & 15) < 4 && k4 < H) put(acc[4], k4);
        STAMP(4)
        if (wv == 3) TRACE(0, s);
      } else if constexpr ((BC == 1 || BC == 2) && MTWMAX == 5) {
        // BC <= 2: all five tiles fit one 16-lane row -- tile t's quad of row b into lane BC t + b by a
        // row shift of BC t (bank mask of that lane group; tiles in increasing order, so a lane a shift
        // filled with a neighbour's unused column is rewritten by the later tile that owns it), ONE store
        const unsigned tag = (unsigned)(s + 1) & 0xFFFFu;
        f32x4 xq = acc[0];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          int v = __float_as_int(xq[c]);
          if constexpr (BC == 2) {
            v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[1][c]), 0x112, 0xF, 0x1, false);  // row_shr:2
            v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[2][c]), 0x114, 0xF, 0x2, false);  // row_shr:4
            v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[3][c]), 0x116, 0xF, 0x2, false);  // row_shr:6
            v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[4][c]), 0x118, 0xF, 0x4, false);  // row_shr:8
          } else {
            v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[1][c]), 0x111, 0xF, 0x1, false);  // row_shr:1
            v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[2][c]), 0x112, 0xF, 0x1, false);  // row_shr:2
            v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[3][c]), 0x113, 0xF, 0x1, false);  // row_shr:3
            v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[4][c]), 0x114, 0xF, 0x2, false);  // row_shr:4
          }
          xq[c] = __int_as_float(v);
        }
        const int p = lane & 15, t = p / BC, bb = p % BC, g = lane >> 4;
        const int k = wv * WSPAN + 16 * t + 4 * g;
        if (p < 5 * BC && k < H) {
          const unsigned r0 = pack24(xq[0]), r1 = pack24(xq[1]), r2 = pack24(xq[2]), r3 = pack24(xq[3]);
          const u32x4 x = {r0 | (r1 << 24), (r1 >> 8) | (tag << 16), r2 | (r3 << 24), (r3 >> 8) | (tag << 16)};
          const int off = (((s & 1) * 2 * NG + w) * BC + bb) * HG + (k >> 1);  // granules
          if (wt)
            __builtin_amdgcn_raw_buffer_store_b128(x, xr, off * 8, 0, 16);  // sc1 write-through (group spans XCDs)
          else
            __builtin_amdgcn_raw_buffer_store_b128(x, xr, off * 8, 0, 0);   // plain: stays in the group's L2
        }
        STAMP(4)
        if (wv == 3) TRACE(0, s);
      } else {  // BC = 8: through the wave-private LDS transpose
      if (col < BC) {
#pragma unroll
        for (int t2 = 0; t2 < MTWMAX; ++t2)
          *reinterpret_cast<f32x4*>(wsw + col * WSP + t2 * 16 + 4 * (lane >> 4)) = acc[t2];
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
      STAMP(4)
      const unsigned tag = (unsigned)(s + 1) & 0xFFFFu;
      constexpr int NQW = BC * WSPAN / 4;  // 16-B quads of this wave
      constexpr int NQI = (NQW + 63) / 64;
      // every quad's LDS read issued before the first is used (one LDS round trip, not one per store:
      // a lane past the wave's quads reads a valid clamped quad and stores nothing)
      float4 vq[NQI];
#pragma unroll
      for (int i = 0; i < NQI; ++i) {
        const int e = min(64 * i + lane, NQW - 1);
        const int bb = e / (WSPAN / 4), kl = 4 * (e % (WSPAN / 4));
        vq[i] = *reinterpret_cast<const float4*>(wsw + bb * WSP + kl);
      }
#pragma unroll
      for (int e0 = 0; e0 < NQW; e0 += 64) {
        const int e = e0 + lane;
        const int bb = e / (WSPAN / 4), k = wv * WSPAN + 4 * (e % (WSPAN / 4));
        if ((NQW % 64 == 0 || e < NQW) && k < H) {
          const float4 v = vq[e0 / 64];
          const unsigned r0 = pack24(v.x), r1 = pack24(v.y), r2 = pack24(v.z), r3 = pack24(v.w);
          const u32x4 x = {r0 | (r1 << 24), (r1 >> 8) | (tag << 16), r2 | (r3 << 24), (r3 >> 8) | (tag << 16)};
          const int off = (((s & 1) * 2 * NG + w) * BC + bb) * HG + (k >> 1);  // granules
          if (wt)
            __builtin_amdgcn_raw_buffer_store_b128(x, xr, off * 8, 0, 16);  // sc1 write-through (group spans XCDs)
          else
            __builtin_amdgcn_raw_buffer_store_b128(x, xr, off * 8, 0, 0);   // plain: stays in the group's L2
        }
      }
      if (wv == 3) TRACE(0, s);
      }
    }
    STAMP(5)
    // this step's dG / dGh, after the publish (off the critical path; issued after B1 of the next
    // step instead they measured slower, 7994 vs 8085 mixtures/s, round 3)
#ifndef BWD_EXP_NO_DG  // timing experiments only (results wrong): the BPTT without its dG stores
    store_dg();
#endif
    STAMP(6)
  }
  // fused bias gradients: this cell's sums over t, one plain store per (row, gate) into the
  // per-row partials (bias_reduce_kernel sums the rows in fixed order: deterministic)
  if (cval && a.dbpart) {
    float* pp = a.dbpart + (long long)(bg * 2 + d) * 2 * GH;
#pragma unroll
    for (int q = 0; q < NGATE; ++q) {
      pp[q * H + cj] = sbi[q];
      pp[GH + q * H + cj] = sbh[q];
    }
  } else if (cval) {
#pragma unroll
    for (int q = 0; q < NGATE; ++q) {
      if (a.dbi) atomicAdd(a.dbi + d * GH + q * H + cj, sbi[q]);
      if (a.dbh) atomicAdd(a.dbh + d * GH + q * H + cj, sbh[q]);
    }
  }
  STAMP_FLUSH
}

namespace {
template <int CELL, int BC>
int launch_bwd_pk_t(const RnnArgs& a, int grid, size_t smem, hipStream_t st) {
  if constexpr (BC == 4) {  // the dH GEMM's split-K slabs summed by the top layer (DL4SS_RNN_DOUT_SLABS)
    if (a.dout_ns == 2) return launch_resident(rnn_bwd_pk_kernel<CELL, 4, 2>, grid, smem, st, a);
    if (a.dout_ns == 3) return launch_resident(rnn_bwd_pk_kernel<CELL, 4, 3>, grid, smem, st, a);
    if (a.dout_ns == 4) return launch_resident(rnn_bwd_pk_kernel<CELL, 4, 4>, grid, smem, st, a);
  }
  return launch_resident(rnn_bwd_pk_kernel<CELL, BC>, grid, smem, st, a);
}
template <int CELL>
int launch_bwd_pk_c(const RnnArgs& a, int BC, int grid, size_t smem, hipStream_t st) {
  switch (BC) {
#ifndef RNN_EXP_MINIMAL
    case 1: return launch_bwd_pk_t<CELL, 1>(a, grid, smem, st);
    case 2: return launch_bwd_pk_t<CELL, 2>(a, grid, smem, st);
    case 8: return launch_bwd_pk_t<CELL, 8>(a, grid, smem, st);
#endif
    case 4: return launch_bwd_pk_t<CELL, 4>(a, grid, smem, st);
    default: return (int)hipErrorInvalidValue;
  }
}
}  // namespace

int launch_bwd_pk(const RnnArgs& a, int cell, int BC, int grid, size_t smem, hipStream_t st) {
  if (a.H > HMAX) return (int)hipErrorInvalidValue;  // the large-H plans are never packed
  return cell == CELL_LSTM ? launch_bwd_pk_c<CELL_LSTM>(a, BC, grid, smem, st)
                           : launch_bwd_pk_c<CELL_GRU>(a, BC, grid, smem, st);
}

}  // namespace dl4ss_rnn
