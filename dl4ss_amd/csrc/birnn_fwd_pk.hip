// Packed forward recurrence of the persistent BiLSTM / BiGRU (bf16 MFMA mode, packed hand-off, optional
// fused input projection: the training step's forward) and its launch selection.  See birnn_common.h.
#include "birnn_common.h"

namespace dl4ss_rnn {

// --------------------------------------------------------------------------
// Forward, bf16 MFMA mode with the PACKED hand-off (the throughput path).
//
// Measured on MI355X (tools/rnn_stamps.py, tools/rnn_trace.py; B = 32, H = 300):
// the one-value-granule kernel (birnn_fwd.hip) spends ~5k of its 6.7k cycles per step in the
// hand-off.  Three changes, each timed:
//  * h crosses workgroups already rounded to bf16 (the consumer rounds it anyway:
//    results are bit-identical), three values per 8-B granule
//      granule = { lo: v0 | v1 << 16, hi: v2 | tag << 16 },  16-bit tag = step + 1,
//    two granules per 16-B store, 8 granules per (batch row, producer);
//  * ONE wave polls, keeping two sweeps in flight (the older one is merged while
//    the newer one travels): hand-off 2.3 -> 1.9 us;
//  * granules written with PLAIN stores and read with `sc1` loads: a plain store
//    lands in the producer XCD's L2, which same-XCD consumers read directly, while an
//    `sc1` store drops the line from L2 and the reader goes to the Infinity Fabric:
//    hand-off 1.9 -> 0.96 us, step 2.68 -> 1.64 us.  A group's workgroups are placed
//    on one XCD (group_of), but placement is speed only, never correctness: at launch
//    start every workgroup of a group publishes its XCC id (group_needs_write_through)
//    and only a group found on ONE XCD uses plain stores; a group that spans XCDs writes
//    every granule `sc1` (the validated write-through form, MI355X_MICROARCH.md, Valid
//    forms R2).  (Round 1 wrote every granule twice, plain + `sc1`, and switched a
//    consumer to the `sc1` copy after a stalled poll: the second store cost ~600 cycles
//    of a BPTT step's publish.)  Every value is validated by its own tag either way.
// Waves (FWD_NPW = 2 polling waves): 0-3 MFMA tiles 0-3 + cell update + publish +
//        saved-state stores; 4 polls, and 7 (FWD_NPW >= 2) and 6 (FWD_NPW == 3) poll too
//        (those waves hold no MFMA tile); the remaining waves of 5-7 run MFMA tiles 4..MT-1
//        and the per-step input prefetch.
// Each MFMA tile runs FWD_MV_CHAINS independent accumulator chains over its k-steps.
// --------------------------------------------------------------------------
// Fused input projection: the step's layer-input rows reach LDS by LDS-DMA (16 B per lane,
// lane-linear 1-KB pieces): item i = b * 80 + c is 16-B chunk c (k = 8c .. 8c + 7) of batch row b
// of the chunk, at element 8 i of a step buffer ([b][640] bf16).  Items past the data (c >= Kin / 8
// rounded up, rows past B, the pad items of the last piece) read a global zero line.
typedef __attribute__((address_space(3))) void lds_void_t;
__device__ __attribute__((aligned(64))) const unsigned g_xzero_line[16] = {0};

// Timing instruments (experiment variant libraries only, results wrong; common.h stops a product build)
#ifndef FWD_EXP_SKIP
#define FWD_EXP_SKIP 0  // skip saved-state stores, bits 1 act, 2 cs, 4 out, 8 outb, 16 hprevb, 32 hprev
#endif
#ifndef FWD_EXP_NOXDMA
#define FWD_EXP_NOXDMA 0  // no x-row DMAs after the prologue
#endif
#if !defined(DL4SS_VARIANT_BUILD) && FWD_EXP_NOXDMA
#error "FWD_EXP_NOXDMA is for tools/variant_lib.py builds only"
#endif

template <int CELL, int BC, int XK = 0>  // XK > 0: fused input projection over XK k-steps of 32
__global__ __launch_bounds__(NT, 1) void rnn_fwd_pk_kernel(RnnArgs a) {
  constexpr bool XW = XK > 0;
  constexpr int NGATE = CELL == CELL_LSTM ? 4 : 3;
  constexpr int KSMAX = HMAX / 32;
  constexpr int SHB = shb_stride(HMAX);  // bf16 row stride of the B image (k >= H stays zero)
  const int H = a.H, T = a.T, J = a.J, NG = a.NG;
  const int R = NGATE * J;
  const int MT = (R + 15) / 16;
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
  const int tile = wv < WPOLL ? wv : wv - 1;
  // With 5 MFMA tiles (LSTM, J = 20) tile 4 runs as two k-step halves on the polling waves 4 and
  // 7 -- idle from B1 to B2 and on SIMDs 0 and 3 -- instead of whole on wave 5, which shares SIMD 1
  // with wave 1's tile (stamps: every wave waited ~285 cycles at B2 for it).  Wave 4 takes the
  // even k-steps, wave 7 the odd ones: exactly the two accumulator chains of a whole-tile matvec
  // (FWD_MV_CHAINS = 2), summed in the same order by the cell lanes -- bitwise the same gates.
  const bool t4h = MT == 5 && FWD_NPW == 2;
  const bool mv = wv != WPOLL && tile < MT && !(t4h && tile == 4);
  const bool mvh = t4h && (wv == WPOLL || wv == 7);
  const int SGS = MT * 16 + 4;  // sgate row stride (floats): 4 batch rows on 4 distinct bank quads (fwd_pk_sgs)

  // h B image [16][SHB]: rows 0..BC-1 are the gathered h, row BC stays zero and every MFMA lane
  // of a row >= BC reads it (one broadcast address instead of 15 - BC zero rows: the matvec's B
  // reads are conflict-free, tools/lds_banks.py)
  unsigned short* shb = reinterpret_cast<unsigned short*>(smem);
  // (lengths that are compile-time values come from birnn_layout.h, through constexpr variables: a call in
  // place is inlined too late to compile to the same code)
  constexpr int SHBN = fwd_shb_n(HMAX), SGXN = fwd_pk_sgx_n(BC), SINN = fwd_pk_sin_n(BC, XW), SPUBN = fwd_pk_spub_bf16(BC);
  float* sgate = smem + SHBN;                    // [BC][SGS]
  float* sgx = sgate + BC * SGS;                 // tile 4's odd-k-step chain (wave 7) [BC][16]; the even one is in sgate
  // per-step input projections [NSIN][sin_slab]: double buffered, or with XW two blocks of SPB steps
  constexpr int SPB = xw_spb(BC);
  constexpr int SINS = sin_slab(BC);
  float* sin = sgx + SGXN;
  // [BC][PKU]: the stage of the round-2..5 publish, unused since the DPP publish (round 6); kept, and
  // zeroed as before, so that the ring below and the compiled kernels stay where they are
  unsigned short* spub = reinterpret_cast<unsigned short*>(sin + SINN);
  // XW: the ring of 3 * SPB step slots of the layer-input rows ([BC][SXB] bf16 + the pad items of
  // the last DMA piece), 256-B aligned (the bank order of its rows)
  static_assert(!XW || FWD_NPW == 2, "the fused projection's DMA pieces assume two prefetch waves of 64 lanes");
  static_assert(16 % BC == 0, "a block fills the MFMA's 16 B-columns");
  constexpr int NXQ = xw_nxq(BC);       // DMA pieces per prefetch wave and step
  constexpr int XSL = xw_slot(BC);      // bf16 per step slot
  constexpr int NSLOT = 3 * SPB;
  // (advanced from spub by element arithmetic, not through an integer cast: the cast lost the LDS
  //  address space and every read of the ring (the projection's B fragments) compiled to a FLAT load,
  //  counted in vmcnt as well as lgkmcnt -- 120 per fused kernel, round 6)
  unsigned short* const sx0 = spub + SPUBN;
  const unsigned sxpad = (256u - ((unsigned)reinterpret_cast<uintptr_t>(sx0) & 255u)) & 255u;
  unsigned short* sxb = sx0 + sxpad / 2;

  // ---- W_hh tile of this wave as bf16 A fragments: lane holds A[row tile*16 + (lane&15)][k]
  bf16x8 afrag[KSMAX];
  {
    const int rl = tile * 16 + (lane & 15);
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
  }
  for (int i = tid; i < SHBN; i += NT) smem[i] = 0.0f;
  for (int i = tid; i < SPUBN; i += NT) spub[i] = 0;

  // ---- XW: the fused projection runs off the cell waves, on waves 4-7 (their slack: the free
  //      prefetch wave 6, the DMA wave 5, and the polling waves between B2 and the first
  //      granule that can land): tile 0 on wave 6, tile 1 on wave 5 (one each: their branch also
  //      holds wave 5's matvec fragments), tiles 2 + 2i on wave 4 and 3 + 2i on wave 7 (two each).
  //      Per tile, bf16 A fragments of its W_ih rows, A[row t*16 + (lane&15)][k = ks*32 +
  //      8(lane>>4) + j] (k >= Kin zero), and the b_ih of the lane's four output rows 4(lane>>4) + i;
  //      loaded inside the roles that use them (dead elsewhere: no register pressure on the cell
  //      waves).  Tile counts per role are compile-time (IC<1> / IC<2>) so unused slots stay dead.
  constexpr int XWT = 2;
  int xt[XWT];
  // second tiles on the prefetch waves, 6 first (600-wide layers 351 us per launch, first layer
  // 313 us; on the polling waves instead: 364 / 327 us, round 3)
  xt[0] = !XW ? -1 : wv == 6 ? 0 : wv == 5 ? 1 : wv == WPOLL ? 2 : wv == 7 ? 3 : -1;
  xt[1] = (XW && (wv == 6 || wv == 5) && xt[0] + 4 < MT) ? xt[0] + 4 : -1;
  if (xt[0] >= MT) xt[0] = -1;
  bf16x8 wfr[XWT][XW ? XK : 1];
  float bir[XWT][4];
  f32x4 xacc[XWT];
  auto load_w = [&](auto ntl) {
    constexpr int NTL = decltype(ntl)::value;
#pragma unroll
    for (int i = 0; i < NTL; ++i) {
      const int t = xt[i];
      const int rl = t * 16 + (lane & 15);
      const int q = rl / J, u = rl % J;
      const bool rv = t >= 0 && rl < R && j0 + u < H;
      const unsigned short* wrow = a.Wihb + ((long long)d * GH + q * H + j0 + u) * a.ldw;
      // one 16-B load per fragment (rows 16-B aligned: ldw % 8 == 0); the chunk holding k = Kin
      // element by element, chunks past it zero
#pragma unroll
      for (int ks = 0; ks < XK; ++ks) {
        const int k0 = ks * 32 + 8 * (lane >> 4);
        if (rv && k0 + 8 <= a.Kin) {
          wfr[i][ks] = *reinterpret_cast<const bf16x8*>(wrow + k0);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) wfr[i][ks][j] = (short)((rv && k0 + j < a.Kin) ? wrow[k0 + j] : 0);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rr = t * 16 + 4 * (lane >> 4) + e;
        const int qq = rr / J, uu = rr % J;
        bir[i][e] = (t >= 0 && rr < R && j0 + uu < H) ? a.bih[(long long)d * GH + qq * H + j0 + uu] : 0.0f;
      }
      xacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  // ---- cell lanes (waves 0-3): row cb = tid / 32, unit cu = tid % 32 (< J)
  const int cb = tid >> 5, cu = tid & 31;
  const bool ct = tid < BC * 32 && cu < J;
  const int cj = j0 + cu;
  const int bg = b0 + cb;
  const bool cval = ct && cj < H && bg < a.B;
  float bh[NGATE];
#pragma unroll
  for (int q = 0; q < NGATE; ++q) bh[q] = cval ? a.bhh[(long long)d * GH + q * H + cj] : 0.0f;
  float hst = 0.0f, cst = 0.0f, hsum = 0.0f;

  // granules of this group: [2 slots][hand-off, spare][BC][NG][8] x 8 B; the spare copy of
  // slot 1 holds the placement granules
  const int slot_g = BC * NG * 8;  // fwd_pk_copy_g
  u64* xg = a.xbuf + (long long)group * PK_NCOPY * slot_g;
  const __amdgpu_buffer_rsrc_t xr = granule_rsrc(xg, (unsigned)(PK_NCOPY * slot_g * 8));
  __shared__ int s_wt;
  if (tid == 0) __hip_atomic_store(xg + PK_PLACE_COPY * slot_g + w, (1ull << 32) | xcc_id(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (wv == WPOLL) {
    const bool wt = group_needs_write_through(xg + PK_PLACE_COPY * slot_g, NG, lane, a.spin_limit, a.status, a.place_force);
    if (lane == 0) s_wt = wt;
  }

  // ---- prefetch waves 5-7 (5-6 with FWD_NPW = 2: wave 7 polls too): input projection
  //      G[b][t][d][q*H + j] of every own (b, unit, gate)
  constexpr int NPF = NT - (WPOLL + FWD_NPW) * 64;  // 192 / 128 prefetch lanes
  const bool pollw = wv == WPOLL || (FWD_NPW >= 2 && wv == 7) || (FWD_NPW == 3 && wv == 6);
  const bool pfw = wv > WPOLL && !pollw;
  constexpr int NQ = (BC * 20 * 4 + NPF - 1) / NPF;
  StepLoader<NQ> ld;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    // item = cell * 4 + gate: consecutive lanes commit consecutive LDS words (conflict-free
    // ds_write_b32; gate-major items were 16 B apart, a 4-way conflict)
    const int i = tid - (WPOLL + 1) * 64 + q * NPF;
    const int gate = i & 3, cell = i >> 2;
    const int ib = b0 + cell / J, iu = cell % J, ij = j0 + iu;
    const bool on = pfw && gate < NGATE && cell < BC * J;
    ld.p[q] = (on && ib < a.B && ij < H) ? a.G + ((long long)ib * T * 2 + d) * GH + gate * H + ij : nullptr;
    ld.stride[q] = 2 * GH;
    ld.shift[q] = 0;
    ld.dst[q] = on ? cell * 4 + gate : -1;
  }
  // XW: per-lane sources of this prefetch wave's DMA pieces (item i = q*128 + (wave-5)*64 + lane)
  const unsigned short* xsrc[NXQ];
  if constexpr (XW) {
#pragma unroll
    for (int q = 0; q < NXQ; ++q) {
      const int i = q * 128 + (wv - WPOLL - 1) * 64 + lane;
      const int b = i / SXC, c = i % SXC;  // chunks c >= 80 of a row are its pad
      const bool on = pfw && b < BC && c < XKMAX * 4 && 8 * c < a.Kin && b0 + b < a.B;
      xsrc[q] = on ? a.Xb + (long long)(b0 + b) * T * a.ldx + 8 * c : nullptr;
    }
  }
  // DMA of step u's rows into ring slot u % NSLOT (prefetch waves only)
  auto xdma = [&](int u) {
    const long long toff = (long long)(d == 0 ? u : T - 1 - u) * a.ldx;
    unsigned short* dst = sxb + (u % NSLOT) * XSL + (wv - WPOLL - 1) * 64 * 8;
#pragma unroll
    for (int q = 0; q < NXQ; ++q) {
      const void* src = xsrc[q] ? (const void*)(xsrc[q] + toff) : (const void*)g_xzero_line;
      __builtin_amdgcn_global_load_lds(src, (lds_void_t*)(dst + q * 128 * 8), 16, 0, 0);
    }
  };
  // wait until at most `n` steps' pieces (the latest issued) are still in flight (n <= SPB)
  auto xwait = [&](int n) {
    static_assert(!XW || SPB * NXQ <= 63, "vmcnt range");
#define XW_WAIT(k) \
  case k:          \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((k) * NXQ <= 63 ? (k) * NXQ : 63) : "memory"); break;
    switch (n) {
      XW_WAIT(0) XW_WAIT(1) XW_WAIT(2) XW_WAIT(3) XW_WAIT(4) XW_WAIT(5) XW_WAIT(6) XW_WAIT(7) XW_WAIT(8)
      XW_WAIT(9) XW_WAIT(10) XW_WAIT(11) XW_WAIT(12) XW_WAIT(13) XW_WAIT(14) XW_WAIT(15)
      default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(16 * NXQ <= 63 ? 16 * NXQ : 63) : "memory");
    }
#undef XW_WAIT
  };
  if (XW && pfw) {
    // blocks 0-2 in flight; blocks 0 and 1 must land before the first barrier (block 0's chain
    // runs before the loop, block 1's first part at step 0)
    for (int u = 0; u < min(T, NSLOT); ++u) xdma(u);
    xwait(max(0, min(T, NSLOT) - 2 * SPB));
  } else if (!XW && pfw) {
    ld.issue(d == 0 ? 0 : T - 1, T);
  }
  __syncthreads();
  const bool wt = __builtin_amdgcn_readfirstlane(s_wt) != 0;  // granules written through (group spans XCDs)
  if (tid == 0) release_start(a.gctl, a.xbuf, ngroups, NG, (long long)PK_NCOPY * slot_g, (long long)PK_PLACE_COPY * slot_g);
  STAMP_DECL

  // XW: G of block kb (steps kb*SPB .. +SPB-1) for this wave's tiles' rows: x W_ih^T as one
  // accumulator chain over the k-steps in order, then + b_ih (the separate GEMM's arithmetic:
  // gemm_gl's k-loop and bias epilogue, bitwise).  xpart runs part j of it, the k-steps
  // [j PK, (j+1) PK) (the B fragments, shared by the wave's tiles, read once; every index
  // compile-time through the unrolled part switch); xfinal adds b_ih and writes the block's G to
  // sin.  B column n = o * BC + b: step kb*SPB + o, batch row b.
  constexpr int PK = XW ? (XK + SPB - 1) / SPB : 1;
  auto xpart = [&](auto ntl, int kb, int j) {
    constexpr int NTL = decltype(ntl)::value;
    if (xt[0] < 0) return;
    const int n = lane & 15;
    const unsigned short* bp = sxb + ((kb % 3) * SPB + n / BC) * XSL + (n % BC) * SXB + 8 * (lane >> 4);
#pragma unroll
    for (int jj = 0; jj < SPB; ++jj) {
      if (jj != j || jj * PK >= XK) continue;
      bf16x8 bv[PK];
#pragma unroll
      for (int i = 0; i < PK; ++i)
        if (jj * PK + i < XK) bv[i] = *reinterpret_cast<const bf16x8*>(bp + (jj * PK + i) * 32);
#pragma unroll
      for (int i = 0; i < PK; ++i)
        if (jj * PK + i < XK) {
#pragma unroll
          for (int t = 0; t < NTL; ++t)
            if (xt[t] >= 0)
              xacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[t][jj * PK + i], bv[i], xacc[t], 0, 0, 0);
        }
    }
  };
  auto xfinal = [&](auto ntl, int kb) {
    constexpr int NTL = decltype(ntl)::value;
    const int n = lane & 15, o = n / BC, b = n % BC;
    float* dst = sin + ((kb & 1) * SPB + o) * SINS;
#pragma unroll
    for (int i = 0; i < NTL; ++i) {
      if (xt[i] < 0) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rr = xt[i] * 16 + 4 * (lane >> 4) + e;
        if (rr < R) dst[(b * J + rr % J) * 4 + rr / J] = xacc[i][e] + bir[i][e];
      }
      xacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  // this step's part of block kb + 1's chain (steps of block kb = s / SPB); the last part finishes it
  auto xstep = [&](auto ntl, int s) {
    const int kb = s / SPB + 1, j = s % SPB;
    if (kb * SPB >= T) return;
    xpart(ntl, kb, j);
    if (j == SPB - 1 || s == T - 1) xfinal(ntl, kb);
  };
  // a role's start: its W_ih fragments, then block 0 whole (its rows landed before the barrier)
  auto xstart = [&](auto ntl) {
    load_w(ntl);
    for (int j = 0; j < SPB; ++j) xpart(ntl, 0, j);
    xfinal(ntl, 0);
  };
  // compile-time tile slots of the prefetch-wave and polling-wave roles
  using XPF = std::integral_constant<int, 2>;
  using XPL = std::integral_constant<int, 1>;

  // tile 4's half on a polling wave: the even (wave 4, into sgate's tile-4 columns) or odd (wave 7,
  // into sgx) k-steps as one accumulator chain in k order; afh[i] holds k-step 2i + (wave 7), loaded
  // inside the polling role (dead in every other role)
  constexpr int KH = (KSMAX + 1) / 2;
  auto load_half = [&](bf16x8* afh) __attribute__((always_inline)) {
    const int rl = 4 * 16 + (lane & 15);
    const int q = rl / J, u = rl % J;
    const bool rv = mvh && rl < R && j0 + u < H;
    const int kpar = wv == 7 ? 1 : 0;
    const float* wrow = a.Whh + ((long long)d * GH + q * H + j0 + u) * H;
#pragma unroll
    for (int i = 0; i < KH; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kk = 2 * i + kpar;
        const int k = kk * 32 + 8 * (lane >> 4) + j;
        afh[i][j] = (short)bf16_rne((rv && kk < KSMAX && k < H) ? wrow[k] : 0.0f);
      }
  };
  auto matvec_half = [&](const bf16x8* afh) __attribute__((always_inline)) {
    const int kpar = wv == 7 ? 1 : 0;
    const unsigned short* bp = shb + min(lane & 15, BC) * SHB + 8 * (lane >> 4) + kpar * 32;
    bf16x8 bv[KH];
#pragma unroll
    for (int i = 0; i < KH; ++i)
      if (2 * i + kpar < KSMAX) bv[i] = *reinterpret_cast<const bf16x8*>(bp + i * 64);
    __builtin_amdgcn_sched_barrier(0);  // every B read before the first MFMA (one LDS round trip)
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KH; ++i)
      if (2 * i + kpar < KSMAX) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afh[i], bv[i], acc, 0, 0, 0);
    const int col = lane & 15;
    if (col < BC) {
      float* dst = wv == 7 ? sgx + col * 16 : sgate + col * SGS + 4 * 16;
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[(lane >> 4) * 4 + i] = acc[i];
    }
  };
  // sgate[b][tile*16 + row] = sum_k W[row][k] h[b][k]
  auto matvec = [&]() __attribute__((always_inline)) {
    if (!mv) return;
    const unsigned short* bp = shb + min(lane & 15, BC) * SHB + 8 * (lane >> 4);
    bf16x8 bv[KSMAX];
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks) bv[ks] = *reinterpret_cast<const bf16x8*>(bp + ks * 32);
    // every B read issued before the first MFMA: one LDS round trip instead of one per pair
    // (the scheduler otherwise interleaves reads and waits to save registers)
    __builtin_amdgcn_sched_barrier(0);
    // FWD_MV_CHAINS independent accumulator chains over the k-steps (the chain length is
    // the matvec's latency), summed in fixed order
    f32x4 acc[FWD_MV_CHAINS];
#pragma unroll
    for (int c = 0; c < FWD_MV_CHAINS; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks)
      acc[ks % FWD_MV_CHAINS] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[ks], bv[ks], acc[ks % FWD_MV_CHAINS], 0, 0, 0);
#pragma unroll
    for (int c = 1; c < FWD_MV_CHAINS; ++c) acc[0] += acc[c];
    const int col = lane & 15;
    if (col < BC) {
#pragma unroll
      for (int i = 0; i < 4; ++i) sgate[col * SGS + tile * 16 + (lane >> 4) * 4 + i] = acc[0][i];
    }
  };

  if (pollw) {
    if (XW) xstart(XPL{});
    bf16x8 afh[KH];
    load_half(afh);
    // ---- polling wave(s): 16-B unit idx = (b * NG + producer) * 4 + pair; lane holds
    //      units lane + 64 (g FWD_NPW + pwv) (idle lanes re-read unit 0: every load is
    //      unconditional, so the compiler can keep a sweep in flight behind a counted vmcnt)
    constexpr int GLK = (BC + FWD_NPW - 1) / FWD_NPW;  // BC * NG * 4 <= 64 * BC  (NG <= 16, checked by the plan)
    const int pwv = wv == WPOLL ? 0 : wv == 7 ? 1 : 2;
    const int n16 = BC * NG * 4;
    int loff[GLK], doff[GLK], dlim[GLK];
#pragma unroll
    for (int g = 0; g < GLK; ++g) {
      const int idx = lane + 64 * (g * FWD_NPW + pwv);
      const bool on = idx < n16;
      const int b = idx / (NG * 4), pw = (idx / 4) % NG, pp = idx % 4;
      const int k0 = pw * J + 6 * pp;
      loff[g] = on ? idx * 16 : 0;
      doff[g] = on ? b * SHB + k0 : 0;
      dlim[g] = on ? max(0, min(min(6, J - 6 * pp), H - k0)) : 0;
    }
    for (int s = 0; s < T; ++s) {
      if (s > 0) {
        const unsigned tag = (unsigned)s & 0xFFFFu;
        const int base = ((s - 1) & 1) * 2 * slot_g * 8;  // the slot's hand-off copy (bytes)
        TRACE(2, s);
        // two sweeps in flight: the older one is merged while the newer one travels;
        // a pair is taken from the first sweep that shows both its tags.  One 16-B `sc1`
        // buffer load per granule pair; the empty asm with a memory clobber before each
        // sweep keeps the loads inside the spin loop (the round-1 8-B relaxed agent atomics were
        // 13-16 % slower per step: DESIGN.md section 5).
        u32x4 v[GLK], qa[GLK], qb[GLK];
        unsigned done = 0;
        asm volatile("" ::: "memory");
#pragma unroll
        for (int g = 0; g < GLK; ++g) qa[g] = __builtin_amdgcn_raw_buffer_load_b128(xr, base + loff[g], 0, 16);
        unsigned spins = 0;
        while (true) {
          asm volatile("" ::: "memory");
#pragma unroll
          for (int g = 0; g < GLK; ++g) qb[g] = __builtin_amdgcn_raw_buffer_load_b128(xr, base + loff[g], 0, 16);
#pragma unroll
          for (int g = 0; g < GLK; ++g) {
            const bool m = ((qa[g].y >> 16) == tag) & ((qa[g].w >> 16) == tag) & !((done >> g) & 1);
            v[g] = m ? qa[g] : v[g];
            done |= (unsigned)m << g;
          }
          if (done == (1u << GLK) - 1) break;
#ifdef RNN_TRACE
          if (spins == 0) TRACE(3, s);
#endif
          asm volatile("" ::: "memory");
#pragma unroll
          for (int g = 0; g < GLK; ++g) qa[g] = __builtin_amdgcn_raw_buffer_load_b128(xr, base + loff[g], 0, 16);
#pragma unroll
          for (int g = 0; g < GLK; ++g) {
            const bool m = ((qb[g].y >> 16) == tag) & ((qb[g].w >> 16) == tag) & !((done >> g) & 1);
            v[g] = m ? qb[g] : v[g];
            done |= (unsigned)m << g;
          }
          if (done == (1u << GLK) - 1) break;
          if (++spins > a.spin_limit) {
            atomicOr(a.status, 1);
            return;
          }
        }
#pragma unroll
        for (int g = 0; g < GLK; ++g) {
          const u32x4 x = v[g];
          unsigned* dst = reinterpret_cast<unsigned*>(shb + doff[g]);  // 4-B aligned: J, H, SHB even
          const int nv = dlim[g];
          if (nv > 0) dst[0] = x.x;
          if (nv > 2) dst[1] = (x.y & 0xFFFFu) | (x.z << 16);
          if (nv > 4) dst[2] = (x.z >> 16) | (x.w << 16);
        }
        TRACE(1, s);
      }
      STAMP(0)
      __syncthreads();  // B1
      STAMP(1)
      if (mvh) matvec_half(afh);
      STAMP(2)
      __syncthreads();  // B2
      STAMP(3)
      // XW: this step's part of the next block's projection, before the next gather: no granule of
      // step s+1 can land before the cell phase and publish that follow B2
      if (XW) xstep(XPL{}, s);
    }
    STAMP_FLUSH
    return;
  }
  if (pfw) {
    // Prefetch waves 5-6.  A wave's role is a compile-time pair (its fused-projection tile slots,
    // whether it holds a matvec tile), so no branch keeps the other role's fragments live: wave 6
    // (two projection tiles at H = 300 LSTM, no matvec) and wave 5 (one projection tile + matvec
    // tile 4) -- one shared body for both kept 2 x XK W_ih fragments and the matvec's W_hh / h
    // fragments live together and spilled 45 VGPRs at XK = 20.
    auto pf_loop = [&](auto ntl, auto with_mv) __attribute__((always_inline)) {
      constexpr bool MV = decltype(with_mv)::value;
      if (XW) xstart(ntl);
      for (int s = 0; s < T; ++s) {
        if (!XW) {
          ld.commit(sin + (s & 1) * SINS);
          if (s + 1 < T) ld.issue(d == 0 ? s + 1 : T - 2 - s, T);
        }
        STAMP(0)
        __syncthreads();  // B1
        STAMP(1)
        if constexpr (MV) matvec();
        // XW: at a block start the rows of the next block (consumed from this step on) landed
        // before B2; the block after it may stay in flight
        if (XW && s % SPB == 0) xwait(max(0, min(SPB, T - (s / SPB + 2) * SPB)));
        STAMP(2)
        __syncthreads();  // B2
        STAMP(3)
        if (XW) xstep(ntl, s);
        // step s + 3 SPB's rows into slot s % NSLOT, issued after B2 (off the matvec -> B2 path; after B1
        // instead: C2 3.540 vs 3.498 ms per step, A/B x3, round 5); that slot held step s's rows, last
        // read by the chain of block s / SPB, which ended before B1(s)
        if (XW && !FWD_EXP_NOXDMA && s + NSLOT < T) xdma(s + NSLOT);
        STAMP(4)
      }
    };
    // (fused projection: wave 6 holds no matvec tile and wave 5 one projection tile --
    // dl4ss_birnn_fwd_xw_supported admits at most 5 MFMA tiles; without it the slot count is moot)
    using XP1 = std::integral_constant<int, 1>;
    if (wv == 6 && !mv)
      pf_loop(XPF{}, std::false_type{});
    else
      pf_loop(XP1{}, std::true_type{});
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
    if (tid < BC * 32) {
      float hn = 0.0f, st[4] = {0.f, 0.f, 0.f, 0.f};
      if (cval) {
        float hg[NGATE], gx[NGATE];
        const int sb = XW ? ((s / SPB) & 1) * SPB + s % SPB : (s & 1);
        const float4 g4 = *reinterpret_cast<const float4*>(sin + sb * SINS + (cb * J + cu) * 4);  // one 16-B read
        const float gxa[4] = {g4.x, g4.y, g4.z, g4.w};
        // tile 4 (rows 64..79: with J = 20 only gate 3's units 4..19): even chain + odd chain, as the
        // whole-tile matvec's acc[0] + acc[1]; read unconditionally (a clamped address) and selected
        const int r3 = (NGATE - 1) * J + cu;
        const float x4 = sgx[cb * 16 + max(r3 - 64, 0)];
        float mqs[NGATE];
#pragma unroll
        for (int q = 0; q < NGATE; ++q) mqs[q] = sgate[cb * SGS + q * J + cu];
#pragma unroll
        for (int q = 0; q < NGATE; ++q) {
          float mq = mqs[q];
          if (q == NGATE - 1) mq = (t4h && r3 >= 64) ? mq + x4 : mq;
          hg[q] = bh[q] + mq;
          gx[q] = gxa[q];
        }
        if constexpr (CELL == CELL_LSTM) {
          const float ig = fsig(gx[0] + hg[0]);
          const float fg = fsig(gx[1] + hg[1]);
          const float gg = ftanh(gx[2] + hg[2]);
          const float og = fsig(gx[3] + hg[3]);
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
      STAMP(5)
      // publish: lane cu = 6 k (k < 4) of each row packs the bf16 h of units cu .. cu + 5 (units >=
      // J and padded rows are zeros) into two tagged granules and stores them with one 16-B
      // write-through store.  The neighbours' values arrive by five DPP wave shifts (lane i reads
      // lane i + 1), not through an LDS stage and read-back (round 6: the LDS round trip sat on
      // every step's critical path)
      {
        const int v0 = ct ? (int)bf16_rne(hn) : 0;
        const int v1 = __builtin_amdgcn_mov_dpp(v0, 0x130, 0xF, 0xF, true);  // wave_shl:1
        const int v2 = __builtin_amdgcn_mov_dpp(v1, 0x130, 0xF, 0xF, true);
        const int v3 = __builtin_amdgcn_mov_dpp(v2, 0x130, 0xF, 0xF, true);
        const int v4 = __builtin_amdgcn_mov_dpp(v3, 0x130, 0xF, 0xF, true);
        const int v5 = __builtin_amdgcn_mov_dpp(v4, 0x130, 0xF, 0xF, true);
        const int k6 = cu / 6;
        if (cu == 6 * k6 && k6 < 4) {
          const unsigned tag = (unsigned)(s + 1) & 0xFFFFu;
          const u32x4 x = {(unsigned)v0 | ((unsigned)v1 << 16), (unsigned)v2 | (tag << 16),
                           (unsigned)v3 | ((unsigned)v4 << 16), (unsigned)v5 | (tag << 16)};
          const int off = ((s & 1) * 2 * slot_g + (cb * NG + w) * 8 + 2 * k6) * 8;
          if (wt)
            __builtin_amdgcn_raw_buffer_store_b128(x, xr, off, 0, 16);  // sc1 write-through (group spans XCDs)
          else
            __builtin_amdgcn_raw_buffer_store_b128(x, xr, off, 0, 0);   // plain: stays in the group's L2
        }
      }
      STAMP(6)
      if (tid == 0) TRACE(0, s);
      // (the saved-state stores leave from the cell lanes right behind the publish: staged in LDS and
      // stored by waves 2-3 during the next step they measured ~14 us slower per launch, round 5)
      if (cval) {
        const long long bt = (long long)bg * T + t;
        // The saved gate activations and cell states (read back only by the BPTT, after the rest of
        // the forward, the loss and the Linear's backward) leave with non-temporal stores: C2
        // 3.438-3.449 vs 3.452-3.472 ms per step (A/B x3 twice, profiles/r05_nt_saves_ab.txt).  Measured
        // and not kept: the bf16 layer output / h_{t-1} copies both non-temporal too (the next GEMMs
        // read the output soon: 3.496-3.508 ms), and the BPTT's bf16 dG as well (3.529-3.532 ms).
        if (FWD_EXP_SKIP & 1) {
        } else if (a.act_cm) {
          typedef float nt_f4 __attribute__((ext_vector_type(4)));
          __builtin_nontemporal_store(nt_f4{st[0], st[1], st[2], st[3]},
                                      reinterpret_cast<nt_f4*>(a.act + ((bt * 2 + d) * H + cj) * 4));
        } else {
          float* actp = a.act + (bt * 2 + d) * (4 * H) + cj;
          actp[0] = st[0]; actp[H] = st[1]; actp[2 * H] = st[2]; actp[3 * H] = st[3];
        }
        if constexpr (CELL == CELL_LSTM)
          if (!(FWD_EXP_SKIP & 2)) __builtin_nontemporal_store(cst, a.cs + (bt * 2 + d) * H + cj);
        const long long ho = bt * 2 * H + d * H + cj;
        if (a.hprev && !(FWD_EXP_SKIP & 32)) a.hprev[ho] = hst;
        if (a.out && !(FWD_EXP_SKIP & 4)) a.out[ho] = hn;
        hsum += hn;
        // bf16 copies, 16-B aligned rows for the GEMMs: out_bf16 (B*T, pad8(2H)) with the
        // directions adjacent (the next layer's K), hprev_bf16 (B*T, 2 pad8(H)) with each
        // direction's block 16-B aligned (the per-direction dW_hh operand)
        const int hp8 = (H + 7) & ~7, op8 = (2 * H + 7) & ~7;
        if (a.outb && !(FWD_EXP_SKIP & 8)) a.outb[bt * op8 + d * H + cj] = bf16_rne(hn);
        // the bf16 h_{t-1} copy (read only by the weight-gradient launch at the end of the backward)
        // non-temporal: 3.440-3.447 vs 3.449-3.454 ms per step (A/B x3, profiles/r05_nt_saves_ab.txt)
        if (a.hprevb && !(FWD_EXP_SKIP & 16))
          __builtin_nontemporal_store((unsigned short)bf16_rne(hst), a.hprevb + bt * 2 * hp8 + d * hp8 + cj);
      }
      hst = hn;
    }
    STAMP(4)
  }
  // the layer output's mean over t (the ADDJUST / classifier time mean, EvalVer.py:363-377): each cell
  // lane's own sum in step order -- no separate pass over the (B, T, 2H) output
  if (a.hmean && cval) a.hmean[(long long)bg * 2 * H + d * H + cj] = hsum / (float)T;
  STAMP_FLUSH
}

namespace {
template <int CELL, int BC>
int launch_fwd_pk_t(const RnnArgs& a, int grid, size_t smem, hipStream_t st) {
  if (a.Xb && a.Kin <= 5 * 32)  // the nets' first layer: 129 features
    return launch_resident(rnn_fwd_pk_kernel<CELL, BC, 5>, grid, smem, st, a);
  if (a.Xb) return launch_resident(rnn_fwd_pk_kernel<CELL, BC, XKMAX>, grid, smem, st, a);
  return launch_resident(rnn_fwd_pk_kernel<CELL, BC>, grid, smem, st, a);
}
template <int CELL>
int launch_fwd_pk_c(const RnnArgs& a, int BC, int grid, size_t smem, hipStream_t st) {
  switch (BC) {
#ifndef RNN_EXP_MINIMAL
    case 1: return launch_fwd_pk_t<CELL, 1>(a, grid, smem, st);
    case 2: return launch_fwd_pk_t<CELL, 2>(a, grid, smem, st);
    case 8: return launch_fwd_pk_t<CELL, 8>(a, grid, smem, st);
#endif
    case 4: return launch_fwd_pk_t<CELL, 4>(a, grid, smem, st);
    default: return (int)hipErrorInvalidValue;
  }
}
}  // namespace

int launch_fwd_pk(const RnnArgs& a, int cell, int BC, int grid, size_t smem, hipStream_t st) {
  if (a.H > HMAX) return (int)hipErrorInvalidValue;
  return cell == CELL_LSTM ? launch_fwd_pk_c<CELL_LSTM>(a, BC, grid, smem, st)
                           : launch_fwd_pk_c<CELL_GRU>(a, BC, grid, smem, st);
}

}  // namespace dl4ss_rnn
