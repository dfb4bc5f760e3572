// Persistent bidirectional LSTM / GRU recurrence for gfx950: the planner, the debug hooks and the C
// ABI (include/dl4ss_hip.h).  The kernels and their launch selection are in birnn_fwd.hip,
// birnn_fwd_pk.hip, birnn_bwd.hip and birnn_bwd_pk.hip; the design is described in birnn_common.h,
// the LDS and workspace layouts in birnn_layout.h.
#include "birnn_common.h"

using namespace dl4ss_rnn;

namespace {

// (the precision flags DL4SS_RNN_WS_ZEROED / _DGH_PAD8 / _DEFER_BIAS / _HARD_GATES / _DOUT_SLABS are the public header's)
constexpr unsigned SPIN_LIMIT = 1u << 20;  // ~1 s of polling: a stuck hand-off exits, never hangs

struct Plan {
  int cell, H;
  int BC, NG, J, nchunk;
  int KP, KPL, HP, RP, RPL, KG, KGL;
  bool fwd_pk;  // packed hand-off forward (rnn_fwd_pk_kernel) applies
  bool bwd_pk;  // packed hand-off BPTT (rnn_bwd_pk_kernel) applies
  bool big;     // H > HMAX: the generic kernels' large-H instantiations (HM = HMAX_L)
  int R() const { return (cell == CELL_LSTM ? 4 : 3) * J; }
  int hm() const { return big ? HMAX_L : HMAX; }
  long long groups() const { return 2LL * nchunk; }
  // dynamic LDS of each kernel (birnn_layout.h); mf: the bf16 MFMA matvec; xw: the fused input projection
  size_t smem_fwd(bool mf) const { return fwd_lds_bytes(mf, hm(), BC, J, R(), HP, KP); }
  // hard: the hard-gates cell runs the runtime-bounds BPTT whatever the plan (the generic maxima)
  size_t smem_bwd(bool mf, bool hard = false) const {
    int rpln = RPLMAX, kgln = KGLMAX;
    if (!hard) bwd_dims(RPL, KGL, rpln, kgln, big);
    return bwd_lds_bytes(mf, hm(), BC, J, NG, RP, RP * rpln, KG * kgln);
  }
  size_t smem_fwd_pk(bool xw) const { return fwd_pk_lds_bytes(BC, R(), xw); }
  size_t smem_bwd_pk() const { return bwd_pk_lds_bytes(BC, J); }
  // the hand-off workspace (birnn_layout.h): bytes a launcher zeroes for its kernel's granules
  long long zero_fwd(bool pk) const {
    return pk ? granule_bytes(groups(), PK_NCOPY, fwd_pk_copy_g(BC, NG)) : granule_bytes(groups(), GEN_NCOPY, fwd_copies_g(1, BC, H));
  }
  long long zero_bwd(bool pk) const {
    return pk ? granule_bytes(groups(), PK_NCOPY, bwd_pk_copy_g(BC, NG, H)) : granule_bytes(groups(), GEN_NCOPY, bwd_copies_g(1, BC, NG, H));
  }
};

// mf: plan for the bf16 MFMA matvec (the fp32 VALU forward's per-thread weight limit
// KPL <= WMAX does not apply).  H > HMAX is the large-H plan (HM = HMAX_L): generic kernels only.
// Co-residency budget of one persistent launch (both directions, all batch chunks): every
// workgroup must be resident at once, so the plan keeps 2 * nchunk * NG within the device's
// CU count minus 1/16 of it (240 of 256 on a full MI355X; 30 on a 32-CU CPX partition),
// leaving room for concurrent kernels (RCCL).
int g_max_wg = 0;  // dl4ss_debug_set_rnn_max_wg (tests force the wider batch chunks)
int wg_limit() {
  if (g_max_wg > 0) return g_max_wg;
  const int cu = device_cu_count();
  return cu > 0 ? cu - cu / 16 : 240;
}

bool make_plan(int cell, int B, int H, Plan& p, bool mf = true, int max_wg = 0) {
  if (H > HMAX_L) return false;
  if (max_wg <= 0) max_wg = wg_limit();
  p.cell = cell;
  p.H = H;
  p.big = H > HMAX;
  const int ngate = cell == CELL_LSTM ? 4 : 3;
  for (int J = 20; J >= 4; --J) {
    const int R = ngate * J;
    if (R > NT) continue;
    const int KP = NT / R;
    int KPL = (H + KP - 1) / KP;
    KPL = (KPL + 3) / 4 * 4;
    if (KPL > WMAX && !mf) continue;
    // bwd: RP row parts x KG k-groups <= NT
    int best_rp = -1, best_kg = 0;
    for (int RP = 1; RP <= 16; ++RP) {
      const int RPL = (R + RP - 1) / RP;
      const int KG = NT / RP;
      const int KGL = (H + KG - 1) / KG;
      if (RPL <= RPLMAX && KGL <= KGLMAX) { best_rp = RP; best_kg = KG; break; }
    }
    if (best_rp < 0) continue;
    const int NG = (H + J - 1) / J;
    if (J > 20) continue;  // gather/publish offset arrays are sized for J <= 20, H <= HMAX(_L)
    int BC = 0;
    for (int bc : {1, 2, 4, 8}) {
      const int nchunk = (B + bc - 1) / bc;
      if (2 * nchunk * NG <= max_wg && bc * J <= NROLE) {
        BC = bc;
        break;
      }
    }
    if (!BC) continue;
    p.BC = BC; p.NG = NG; p.J = J; p.nchunk = (B + BC - 1) / BC;
    p.KP = KP; p.KPL = KPL; p.HP = KP * KPL;
    p.RP = best_rp; p.RPL = (R + best_rp - 1) / best_rp; p.KG = best_kg; p.KGL = (H + best_kg - 1) / best_kg;
    // the packed forward's MFMA tiles must leave its FWD_NPW polling waves free (8 waves, one without a tile)
    p.fwd_pk = !p.big && J % 2 == 0 && H % 2 == 0 && J <= PKU && NG <= 16 && mfma_tiles(R) <= 8 - FWD_NPW;
    p.bwd_pk = !p.big && J % 4 == 0 && H % 4 == 0 && NG <= 16;
    return true;
  }
  return false;
}

// act layout of a plan: cell-major (B,T,2,H,4) when both packed kernels run it at BC >= 4 (the
// forward's one 16-B store per cell, the BPTT's one 16-B load; RnnArgs::act_cm), else gate-major
bool act_cell_major(const Plan& p) { return p.fwd_pk && p.bwd_pk && p.BC >= 4; }

#if defined(RNN_STAMPS) || defined(RNN_TRACE)
u64* g_stamps = nullptr;
#endif

unsigned g_spin_limit = SPIN_LIMIT;  // dl4ss_debug_set_spin_limit (tests force a hand-off timeout)
int g_place_force = 0;               // dl4ss_debug_set_place_force (tests force write-through granules)

void fill_args(RnnArgs& a, const Plan& p, int B, int T, int H) {
  a.spin_limit = g_spin_limit;
  a.place_force = g_place_force;
#if defined(RNN_STAMPS) || defined(RNN_TRACE)
  a.stamps = g_stamps;
#endif
  a.B = B; a.T = T; a.H = H; a.J = p.J; a.NG = p.NG; a.nchunk = p.nchunk;
  a.KP = p.KP; a.KPL = p.KPL; a.HP = p.HP;
  a.RP = p.RP; a.RPL = p.RPL; a.KG = p.KG; a.KGL = p.KGL;
}

// one recurrence launch of a plan through its kernel file's entry (pk: the packed kernels, bf16 only)
// hard: Keras 1's hard_sigmoid gates (generic fp32 LSTM kernels only)
int launch(bool fwd, bool mf, bool pk, const Plan& p, const RnnArgs& a, size_t smem, hipStream_t st, bool hard = false) {
  const int grid = (int)(p.groups() * p.NG);
  if (hard && (pk || mf)) return (int)hipErrorInvalidValue;
  const int e = fwd ? (pk ? launch_fwd_pk(a, p.cell, p.BC, grid, smem, st) : launch_fwd(a, p.cell, p.BC, mf, hard, grid, smem, st))
                    : (pk ? launch_bwd_pk(a, p.cell, p.BC, grid, smem, st) : launch_bwd(a, p.cell, p.BC, mf, hard, grid, smem, st));
  if (e) return e;
  DL4SS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

#if defined(RNN_STAMPS) || defined(RNN_TRACE)
DL4SS_API void dl4ss_debug_set_stamps(void* p) { g_stamps = reinterpret_cast<unsigned long long*>(p); }
#endif

// dbi[i] += sum_b part[b][d][0][g], dbh[i] += sum_b part[b][d][1][g] for i = d * GH + g, rows
// in order b = 0 .. B-1 (the BPTT kernel's per-row bias sums); blockIdx.y = the job (layer)
constexpr int BIAS_JOBS_MAX = 8;
struct BiasJobs {
  int n, B, GH;
  float beta;  // db = beta db + sums (beta 0: written, not read)
  const float* part[BIAS_JOBS_MAX];
  float* dbi[BIAS_JOBS_MAX];
  float* dbh[BIAS_JOBS_MAX];
};
__global__ __launch_bounds__(256) void bias_reduce_kernel(BiasJobs j) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int B = j.B, GH = j.GH;
  if (i >= 2 * GH) return;
  const float* part = j.part[0];
  float* dbi = j.dbi[0];
  float* dbh = j.dbh[0];
#pragma unroll
  for (int k = 1; k < BIAS_JOBS_MAX; ++k)
    if (k == (int)blockIdx.y) { part = j.part[k]; dbi = j.dbi[k]; dbh = j.dbh[k]; }
  const int d = i / GH, g = i - d * GH;
  float si = 0.0f, sh = 0.0f;
  // rows in chunks of 32 with every load of a chunk issued before its adds (a row-by-row
  // loop paid one dependent L2 round trip per row: 12 us per launch at B = 32; chunks of 8, four
  // rounds: 5.6 us; round 6: one round at B <= 32), the sums in row order
  for (int b0 = 0; b0 < B; b0 += 32) {
    float vi[32], vh[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const int b = min(b0 + u, B - 1);
      const float* pp = part + (long long)(b * 2 + d) * 2 * GH + g;
      vi[u] = pp[0];
      vh[u] = pp[GH];
    }
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      si = b0 + u < B ? si + vi[u] : si;
      sh = b0 + u < B ? sh + vh[u] : sh;
    }
  }
  if (dbi) dbi[i] = j.beta != 0.f ? si + j.beta * dbi[i] : si;
  if (dbh) dbh[i] = j.beta != 0.f ? sh + j.beta * dbh[i] : sh;
}

// hand-off area of the BPTT / forward workspace, 256-B aligned
static long long handoff_bytes(const Plan& p, int H);

// per-row bias partials behind the hand-off area (BPTT with fused bias gradients)
static long long bias_part_bytes(const Plan& p, int H) {
  return p.big ? 0 : (long long)p.nchunk * p.BC * 2 * 2 * 4 * H * 4;
}

static long long workspace_bytes(const Plan& p, int H) { return handoff_bytes(p, H) + bias_part_bytes(p, H); }

static long long handoff_bytes(const Plan& p, int H) { return handoff_area_bytes(p.groups(), p.BC, p.NG, H, p.big); }

// the packed kernels' group-formation counters: the last 256 B of the hand-off area (group_pk)
static long long ctl_offset(const Plan& p, int H) { return ctl_offset_bytes(p.groups(), p.BC, p.NG, H); }

// Polls a hand-off may spin before it times out (sets *status and the polling wave exits;
// the launch still completes).  0 restores the default (SPIN_LIMIT, ~1 s).  Test hook: a
// tiny limit forces the timeout path that the Adam guard (dl4ss_adam_guarded) must catch.
DL4SS_API void dl4ss_debug_set_spin_limit(unsigned limit) { g_spin_limit = limit ? limit : SPIN_LIMIT; }

// 1: the packed kernels write every granule through (`sc1`) as if the group spanned XCDs (test
// hook for the cross-XCD form); 0: plain stores wherever the group was found on one XCD.
DL4SS_API void dl4ss_debug_set_place_force(int force) { g_place_force = force == 1 ? 1 : 0; }

// > 0: the co-residency budget of every later plan (max_wg of dl4ss_birnn_plan_info, in
// workgroups) instead of the device's; 0 restores the default.  Test hook: a budget of 120 makes
// the B = 32, H = 300 nets plan batch chunks of 8 (the plan a B >= 33 batch gets on a full part).
DL4SS_API void dl4ss_debug_set_rnn_max_wg(int max_wg) { g_max_wg = max_wg > 0 ? max_wg : 0; }

// The recurrence plan for (cell, B, H) under a co-residency budget of max_wg workgroups
// (<= 0: the current device's, see wg_limit): info = {BC, NG, J, nchunk, grid}.  Host-only
// (no device call when max_wg > 0).  Returns 0, or hipErrorInvalidValue when no plan fits.
DL4SS_API int dl4ss_birnn_plan_info(int cell, int B, int H, int precision, int max_wg, int* info) {
  DL4SS_REQUIRE(info && (cell == CELL_LSTM || cell == CELL_GRU) && B > 0 && H > 0);
  Plan p;
  if (!make_plan(cell, B, H, p, precision == 1, max_wg)) return (int)hipErrorInvalidValue;
  info[0] = p.BC; info[1] = p.NG; info[2] = p.J; info[3] = p.nchunk; info[4] = 2 * p.nchunk * p.NG;
  return 0;
}

// Sub-batch of a forward whose plan does not fit the co-residency budget at B: the fp32 VALU
// plan of a wide layer (H = 600, the classifier: J <= 12, 50 workgroups per group) fits at most
// B = 16 on a full part.  Rows never interact, so dl4ss_birnn_fwd_mean runs such a batch as
// consecutive launches of (near-)equal sub-batches.  0 when no sub-batch fits either.
static int split_batch(int cell, int B, int H, bool mf, Plan& ps) {
  int fit = 0;
  for (int b = B - 1; b >= 1 && !fit; --b)
    if (make_plan(cell, b, H, ps, mf)) fit = b;
  if (!fit) return 0;
  const int n = (B + fit - 1) / fit;
  const int bs = (B + n - 1) / n;
  return make_plan(cell, bs, H, ps, mf) ? bs : 0;
}

// the larger of the fp32 and bf16 plans' needs (either precision may use the buffer; an fp32
// forward planned as sub-batches counts its sub-batch plan); -1 when neither plan exists
DL4SS_API long long dl4ss_birnn_workspace_bytes(int cell, int B, int H) {
  long long best = -1;
  for (bool mf : {false, true}) {
    Plan p;
    if (!make_plan(cell, B, H, p, mf) && (mf || split_batch(cell, B, H, mf, p) == 0)) continue;
    const long long n = workspace_bytes(p, H);
    if (n > best) best = n;
  }
  return best;
}

DL4SS_API int dl4ss_birnn_fwd_ex(int cell, int precision, int B, int T, int H, const float* G, const float* W_hh,
                                 const float* b_hh, float* out, float* hprev, float* act, float* cs, void* out_bf16,
                                 void* hprev_bf16, void* workspace, long long ws_bytes, int* status, void* stream);

DL4SS_API int dl4ss_birnn_fwd(int cell, int precision, int B, int T, int H, const float* G, const float* W_hh, const float* b_hh,
                              float* out, float* hprev, float* act, float* cs, void* workspace,
                              long long ws_bytes, int* status, void* stream) {
  DL4SS_REQUIRE(hprev);
  return dl4ss_birnn_fwd_ex(cell, precision, B, T, H, G, W_hh, b_hh, out, hprev, act, cs, nullptr, nullptr, workspace,
                            ws_bytes, status, stream);
}

DL4SS_API int dl4ss_birnn_fwd_mean(int cell, int precision, int B, int T, int H, const float* G, const float* W_hh,
                                   const float* b_hh, float* out, float* hprev, float* act, float* cs, void* out_bf16,
                                   void* hprev_bf16, float* h_mean, void* workspace, long long ws_bytes, int* status,
                                   void* stream);

DL4SS_API int dl4ss_birnn_fwd_ex(int cell, int precision, int B, int T, int H, const float* G, const float* W_hh,
                                 const float* b_hh, float* out, float* hprev, float* act, float* cs, void* out_bf16,
                                 void* hprev_bf16, void* workspace, long long ws_bytes, int* status, void* stream) {
  DL4SS_REQUIRE(out);
  return dl4ss_birnn_fwd_mean(cell, precision, B, T, H, G, W_hh, b_hh, out, hprev, act, cs, out_bf16, hprev_bf16,
                              nullptr, workspace, ws_bytes, status, stream);
}

// dl4ss_birnn_fwd_ex with the fp32 output optional (packed kernel: out may be NULL when out_bf16 is
// not) and the time mean of the output formed in the recurrence (h_mean, packed kernel only)
DL4SS_API int dl4ss_birnn_fwd_mean(int cell, int precision, int B, int T, int H, const float* G, const float* W_hh,
                                   const float* b_hh, float* out, float* hprev, float* act, float* cs, void* out_bf16,
                                   void* hprev_bf16, float* h_mean, void* workspace, long long ws_bytes, int* status,
                                   void* stream) {
  DL4SS_REQUIRE(cell == CELL_LSTM || cell == CELL_GRU);
  const bool prezeroed = precision & DL4SS_RNN_WS_ZEROED;  // the caller zeroed the workspace (one fill per step)
  const bool hard = precision & DL4SS_RNN_HARD_GATES;  // Keras 1's cell: fp32 LSTM, generic kernel, no bf16 extras
  precision &= ~(DL4SS_RNN_WS_ZEROED | DL4SS_RNN_HARD_GATES);
  DL4SS_REQUIRE(precision == 0 || precision == 1);
  DL4SS_REQUIRE(!hard || (cell == CELL_LSTM && precision == 0 && out && !out_bf16 && !hprev_bf16 && !h_mean));
  DL4SS_REQUIRE(B > 0 && T > 0 && H > 0 && G && W_hh && b_hh && (out || out_bf16) && act && workspace && status);
  DL4SS_REQUIRE(cell == CELL_GRU || cs);
  Plan p;
  if (precision == 0 && !make_plan(cell, B, H, p, false)) {
    // the fp32 plan does not fit at this batch: consecutive sub-batch launches (split_batch),
    // each zeroing the shared hand-off workspace itself (stream order keeps them apart)
    const int bs = split_batch(cell, B, H, false, p);
    DL4SS_REQUIRE(bs > 0 && out && !h_mean && !out_bf16 && !hprev_bf16);
    const long long GH = (cell == CELL_LSTM ? 4LL : 3LL) * H;
    for (int b0 = 0; b0 < B; b0 += bs) {
      const long long r = (long long)b0 * T;  // (b, t) rows before the sub-batch
      const int rc = dl4ss_birnn_fwd_mean(cell, hard ? DL4SS_RNN_HARD_GATES : 0, B - b0 < bs ? B - b0 : bs, T, H, G + r * 2 * GH, W_hh, b_hh,
                                          out + r * 2 * H, hprev ? hprev + r * 2 * H : nullptr, act + r * 2 * 4 * H,
                                          cs ? cs + r * 2 * H : nullptr, nullptr, nullptr, nullptr, workspace,
                                          ws_bytes, status, stream);
      if (rc) return rc;
    }
    return 0;
  }
  DL4SS_REQUIRE(make_plan(cell, B, H, p, precision == 1));
  DL4SS_REQUIRE(ws_bytes >= workspace_bytes(p, H));
  hipStream_t st = as_stream(stream);
  const bool mf = precision == 1;
  const bool pk = mf && p.fwd_pk && T < 65535;
  const bool act_cm = pk && act_cell_major(p);
  DL4SS_REQUIRE(pk || (out && !h_mean));  // the optional output and the fused mean are the packed kernel's
  if (!prezeroed) {
    hipError_t e = hipMemsetAsync(workspace, 0, p.zero_fwd(pk), st);
    if (e == hipSuccess && pk) e = hipMemsetAsync(static_cast<char*>(workspace) + ctl_offset(p, H), 0, CTL_BYTES, st);
    if (e != hipSuccess) return (int)e;
  }
  // the bf16 copies, and dropping the fp32 h_{t-1} (only the GRU BPTT reads it), need the packed kernel
  DL4SS_REQUIRE(pk || (!out_bf16 && !hprev_bf16 && hprev));
  DL4SS_REQUIRE(hprev || cell == CELL_LSTM);
  RnnArgs a{};
  fill_args(a, p, B, T, H);
  a.G = G; a.Whh = W_hh; a.bhh = b_hh; a.out = out; a.hprev = hprev; a.act = act; a.cs = cs;
  a.act_cm = act_cm ? 1 : 0;
  a.hmean = h_mean;
  a.outb = reinterpret_cast<unsigned short*>(out_bf16);
  a.hprevb = reinterpret_cast<unsigned short*>(hprev_bf16);
  a.xbuf = reinterpret_cast<unsigned long long*>(workspace);
  a.gctl = pk ? reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + ctl_offset(p, H)) : nullptr;
  a.status = status;
  return launch(true, mf, pk, p, a, pk ? p.smem_fwd_pk(false) : p.smem_fwd(mf), st, hard);
}

// 1 when the packed bf16 forward (the only one with the fused input projection) applies to
// (cell, B, H, T) and the layer input width Kin: dl4ss_birnn_fwd_xw may be called
DL4SS_API int dl4ss_birnn_fwd_xw_supported(int cell, int B, int T, int H, int Kin) {
  if (!(cell == CELL_LSTM || cell == CELL_GRU) || B <= 0 || T <= 0 || H <= 0 || Kin <= 0) return 0;
  Plan p;
  if (!make_plan(cell, B, H, p, true)) return 0;
  // at most 5 MFMA tiles (R <= 80 gate rows): prefetch wave 6 then holds no matvec tile and wave 5
  // one projection tile, the compile-time roles of rnn_fwd_pk_kernel's prefetch branch
  const int ngate = cell == CELL_LSTM ? 4 : 3;
  return (p.fwd_pk && T < 65535 && Kin <= XKMAX * 32 && (ngate * p.J + 15) / 16 <= 5) ? 1 : 0;
}

// dl4ss_birnn_fwd_ex with the input projection fused into the recurrence (bf16 mode only): instead
// of reading G = X W_ih^T + b_ih from a separate GEMM, every workgroup forms its own gate rows of
// step t+1 with MFMAs while step t's hand-off travels.  x_bf16: (B*T, ldx) bf16 layer input rows
// (16-B chunks: padding up to the next multiple of 8 finite); W_ih_bf16: (2*NGATE*H, ldw) bf16 (direction-major rows, the GEMM's B operand); b_ih
// (2, NGATE*H) fp32.  ldx, ldw multiples of 8 and both bases 16-B aligned.  Same summation order as
// the GEMM path (one k-ordered MFMA chain, then + b_ih): the outputs match it bit for bit.
DL4SS_API int dl4ss_birnn_fwd_xw_ex(int cell, int B, int T, int H, const void* x_bf16, int Kin, long long ldx,
                                    const void* W_ih_bf16, long long ldw, const float* b_ih, const float* W_hh,
                                    const float* b_hh, float* out, float* hprev, float* act, float* cs,
                                    void* out_bf16, void* hprev_bf16, float* h_mean, void* workspace,
                                    long long ws_bytes, int* status, void* stream, int ws_zeroed);

DL4SS_API int dl4ss_birnn_fwd_xw(int cell, int B, int T, int H, const void* x_bf16, int Kin, long long ldx,
                                 const void* W_ih_bf16, long long ldw, const float* b_ih, const float* W_hh,
                                 const float* b_hh, float* out, float* hprev, float* act, float* cs, void* out_bf16,
                                 void* hprev_bf16, void* workspace, long long ws_bytes, int* status, void* stream,
                                 int ws_zeroed) {
  DL4SS_REQUIRE(out);
  return dl4ss_birnn_fwd_xw_ex(cell, B, T, H, x_bf16, Kin, ldx, W_ih_bf16, ldw, b_ih, W_hh, b_hh, out, hprev, act, cs,
                               out_bf16, hprev_bf16, nullptr, workspace, ws_bytes, status, stream, ws_zeroed);
}

DL4SS_API int dl4ss_birnn_fwd_xw_ex(int cell, int B, int T, int H, const void* x_bf16, int Kin, long long ldx,
                                    const void* W_ih_bf16, long long ldw, const float* b_ih, const float* W_hh,
                                    const float* b_hh, float* out, float* hprev, float* act, float* cs,
                                    void* out_bf16, void* hprev_bf16, float* h_mean, void* workspace,
                                    long long ws_bytes, int* status, void* stream, int ws_zeroed) {
  DL4SS_REQUIRE(dl4ss_birnn_fwd_xw_supported(cell, B, T, H, Kin));
  DL4SS_REQUIRE(x_bf16 && W_ih_bf16 && b_ih && W_hh && b_hh && act && workspace && status);
  DL4SS_REQUIRE(out || out_bf16);  // some output of the layer
  DL4SS_REQUIRE(cell == CELL_GRU || cs);
  DL4SS_REQUIRE(hprev || cell == CELL_LSTM);
  DL4SS_REQUIRE(ldx >= Kin && ldw >= Kin && ldx % 8 == 0 && ldw % 8 == 0);
  DL4SS_REQUIRE((reinterpret_cast<uintptr_t>(x_bf16) & 15) == 0 && (reinterpret_cast<uintptr_t>(W_ih_bf16) & 15) == 0);
  Plan p;
  DL4SS_REQUIRE(make_plan(cell, B, H, p, true));
  DL4SS_REQUIRE(ws_bytes >= workspace_bytes(p, H));
  hipStream_t st = as_stream(stream);
  if (!ws_zeroed) {
    hipError_t e = hipMemsetAsync(workspace, 0, p.zero_fwd(true), st);
    if (e == hipSuccess) e = hipMemsetAsync(static_cast<char*>(workspace) + ctl_offset(p, H), 0, CTL_BYTES, st);
    if (e != hipSuccess) return (int)e;
  }
  RnnArgs a{};
  fill_args(a, p, B, T, H);
  a.G = nullptr; a.Whh = W_hh; a.bhh = b_hh; a.out = out; a.hprev = hprev; a.act = act; a.cs = cs;
  a.act_cm = act_cell_major(p) ? 1 : 0;
  a.hmean = h_mean;
  a.outb = reinterpret_cast<unsigned short*>(out_bf16);
  a.hprevb = reinterpret_cast<unsigned short*>(hprev_bf16);
  a.xbuf = reinterpret_cast<unsigned long long*>(workspace);
  a.gctl = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + ctl_offset(p, H));
  a.status = status;
  a.Xb = reinterpret_cast<const unsigned short*>(x_bf16);
  a.Wihb = reinterpret_cast<const unsigned short*>(W_ih_bf16);
  a.bih = b_ih;
  a.Kin = Kin; a.ldx = ldx; a.ldw = ldw;
  return launch(true, true, true, p, a, p.smem_fwd_pk(true), st);
}

DL4SS_API int dl4ss_birnn_bwd_ex(int cell, int precision, int B, int T, int H, const float* dOut,
                                 const float* dOut_bcast, const float* W_hh, const float* act, const float* cs,
                                 const float* hprev, float* dG, float* dGh, void* dG_bf16, void* dGh_bf16,
                                 float* db_ih, float* db_hh, void* workspace, long long ws_bytes, int* status,
                                 void* stream);

DL4SS_API int dl4ss_birnn_bwd(int cell, int precision, int B, int T, int H, const float* dOut, const float* dOut_bcast,
                              const float* W_hh, const float* act, const float* cs, const float* hprev, float* dG,
                              float* dGh, void* workspace, long long ws_bytes, int* status, void* stream) {
  DL4SS_REQUIRE(dG && (cell == CELL_LSTM || dGh));
  DL4SS_REQUIRE(H <= HMAX && dOut);  // the mask nets' entry point; H <= HMAX_L: dl4ss_birnn_bwd_ex
  return dl4ss_birnn_bwd_ex(cell, precision, B, T, H, dOut, dOut_bcast, W_hh, act, cs, hprev, dG, dGh, nullptr,
                            nullptr, nullptr, nullptr, workspace, ws_bytes, status, stream);
}

DL4SS_API int dl4ss_birnn_bwd_ex(int cell, int precision, int B, int T, int H, const float* dOut,
                                 const float* dOut_bcast, const float* W_hh, const float* act, const float* cs,
                                 const float* hprev, float* dG, float* dGh, void* dG_bf16, void* dGh_bf16,
                                 float* db_ih, float* db_hh, void* workspace, long long ws_bytes, int* status,
                                 void* stream) {
  DL4SS_REQUIRE(cell == CELL_LSTM || cell == CELL_GRU);
  const bool prezeroed = precision & DL4SS_RNN_WS_ZEROED;
  const bool dgh_pad8 = precision & DL4SS_RNN_DGH_PAD8;
  const bool defer_bias = precision & DL4SS_RNN_DEFER_BIAS;
  const bool hard = precision & DL4SS_RNN_HARD_GATES;  // Keras 1's cell: fp32 LSTM, generic kernel, no bf16 extras
  const int dout_ns = ((precision & DL4SS_RNN_DOUT_SLABS_MASK) >> 12) + 1;
  precision &= ~(DL4SS_RNN_WS_ZEROED | DL4SS_RNN_DGH_PAD8 | DL4SS_RNN_DEFER_BIAS | DL4SS_RNN_HARD_GATES | DL4SS_RNN_DOUT_SLABS_MASK);
  DL4SS_REQUIRE(precision == 0 || precision == 1);
  DL4SS_REQUIRE(!hard || (cell == CELL_LSTM && precision == 0 && dout_ns == 1 && dG && !dG_bf16 && !dGh_bf16));
  DL4SS_REQUIRE(B > 0 && T > 0 && H > 0 && H <= HMAX_L && W_hh && act && workspace && status);
  // the classifier's top layer: its only gradient is d(mean_t h), so dOut may be NULL (read as zero) when
  // dOut_bcast is given -- in the generic kernel (every H > HMAX plan), checked below
  DL4SS_REQUIRE(dOut || dOut_bcast);
  DL4SS_REQUIRE(dG || dG_bf16);
  DL4SS_REQUIRE(cell == CELL_GRU ? ((dGh || dGh_bf16) && hprev) : (cs != nullptr));
  Plan p;
  if (precision == 0 && H > HMAX && !make_plan(cell, B, H, p, false)) {
    // the wide layer's fp32 plan does not fit at this batch: consecutive sub-batch launches of the
    // forward's sub-batch size (split_batch; rows never interact), each zeroing the shared hand-off
    // workspace itself (stream order keeps them apart)
    const int bs = split_batch(cell, B, H, false, p);
    DL4SS_REQUIRE(bs > 0 && dout_ns == 1 && dG && !dG_bf16 && !dGh_bf16 && !db_ih && !db_hh && (cell == CELL_LSTM || dGh));
    const long long GH = (cell == CELL_LSTM ? 4LL : 3LL) * H;
    for (int b0 = 0; b0 < B; b0 += bs) {
      const long long r = (long long)b0 * T;  // (b, t) rows before the sub-batch
      const int rc = dl4ss_birnn_bwd_ex(cell, hard ? DL4SS_RNN_HARD_GATES : 0, B - b0 < bs ? B - b0 : bs, T, H, dOut ? dOut + r * 2 * H : nullptr,
                                        dOut_bcast ? dOut_bcast + (long long)b0 * 2 * H : nullptr, W_hh,
                                        act + r * 2 * 4 * H, cs ? cs + r * 2 * H : nullptr,
                                        hprev ? hprev + r * 2 * H : nullptr, dG + r * 2 * GH,
                                        dGh ? dGh + r * 2 * GH : nullptr, nullptr, nullptr, nullptr, nullptr, workspace,
                                        ws_bytes, status, stream);
      if (rc) return rc;
    }
    return 0;
  }
  DL4SS_REQUIRE(make_plan(cell, B, H, p, precision == 1));
  DL4SS_REQUIRE(ws_bytes >= workspace_bytes(p, H));
  hipStream_t st = as_stream(stream);
  const bool mf = precision == 1;
  // the packed BPTT at BC >= 4 reads the cell-major act that only the packed forward writes
  const bool pk = mf && p.bwd_pk && T < 65535 && (p.BC < 4 || act_cell_major(p));
  // every refusal comes before the first device call (the workspace fill below)
  DL4SS_REQUIRE(dOut || !pk);  // the packed kernel's step loader reads dOut unconditionally
  // bf16 gradient copies, dropping the fp32 ones and the fused bias sums need the packed kernel
  DL4SS_REQUIRE(pk || (!dG_bf16 && !dGh_bf16 && !db_ih && !db_hh && dG && (cell == CELL_LSTM || dGh)));
  // split-K dOut slabs: the packed BPTT's step-factor prefetch at batch chunks of 4 sums them
  DL4SS_REQUIRE(dout_ns == 1 || (pk && p.BC == 4));
  if (!prezeroed) {
    hipError_t e = hipMemsetAsync(workspace, 0, p.zero_bwd(pk), st);
    if (e == hipSuccess && pk) e = hipMemsetAsync(static_cast<char*>(workspace) + ctl_offset(p, H), 0, CTL_BYTES, st);
    if (e != hipSuccess) return (int)e;
  }
  RnnArgs a{};
  fill_args(a, p, B, T, H);
  a.Whh = W_hh; a.act = const_cast<float*>(act); a.cs = const_cast<float*>(cs);
  a.hprev = const_cast<float*>(hprev); a.dOut = dOut; a.dOutB = dOut_bcast; a.dG = dG; a.dGh = dGh;
  a.dout_ns = dout_ns;
  a.dout_zs = (long long)B * T * 2 * H;
  a.dGb = reinterpret_cast<unsigned short*>(dG_bf16); a.dGhb = reinterpret_cast<unsigned short*>(dGh_bf16);
  const int GHc = (cell == CELL_LSTM ? 4 : 3) * H;
  a.ghb = dgh_pad8 ? (GHc + 7) / 8 * 8 : GHc;
  a.dbi = db_ih; a.dbh = db_hh;
  a.xbuf = reinterpret_cast<unsigned long long*>(workspace);
  a.gctl = pk ? reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + ctl_offset(p, H)) : nullptr;
  const bool bias = pk && (db_ih || db_hh);
  a.dbpart = bias ? reinterpret_cast<float*>(static_cast<char*>(workspace) + handoff_bytes(p, H)) : nullptr;
  a.status = status;
  const int e = launch(false, mf, pk, p, a, pk ? p.smem_bwd_pk() : p.smem_bwd(mf, hard), st, hard);
  if (e || !bias || defer_bias) return e;
  const int GH = (cell == CELL_LSTM ? 4 : 3) * H;
  BiasJobs j{};
  j.n = 1; j.B = B; j.GH = GH; j.beta = 1.f; j.part[0] = a.dbpart; j.dbi[0] = db_ih; j.dbh[0] = db_hh;
  hipLaunchKernelGGL(bias_reduce_kernel, dim3((2 * GH + 255) / 256, 1), dim3(256), 0, st, j);
  return (int)hipGetLastError();
}

// The deferred form: the bias partials of n BPTT launches (DL4SS_RNN_DEFER_BIAS) reduced by ONE
// launch after the last of them -- the per-layer reduce was a 5 us latency-bound launch between
// each BPTT and the input-gradient GEMM that the next BPTT waits on.
DL4SS_API int dl4ss_birnn_bias_reduce_ex(int cell, int B, int H, int n, void* const* workspaces,
                                         float* const* db_ih, float* const* db_hh, float beta, void* stream) {
  DL4SS_REQUIRE((cell == CELL_LSTM || cell == CELL_GRU) && B > 0 && H > 0 && n >= 1 && n <= BIAS_JOBS_MAX);
  DL4SS_REQUIRE(workspaces && db_ih && db_hh);
  Plan p;
  if (!make_plan(cell, B, H, p, true)) return (int)hipErrorInvalidValue;  // the bf16 BPTT's plan
  const int GH = (cell == CELL_LSTM ? 4 : 3) * H;
  BiasJobs j{};
  j.n = n; j.B = B; j.GH = GH; j.beta = beta;
  for (int i = 0; i < n; ++i) {
    DL4SS_REQUIRE(workspaces[i] && db_ih[i] && db_hh[i]);
    j.part[i] = reinterpret_cast<const float*>(static_cast<const char*>(workspaces[i]) + handoff_bytes(p, H));
    j.dbi[i] = db_ih[i];
    j.dbh[i] = db_hh[i];
  }
  hipLaunchKernelGGL(bias_reduce_kernel, dim3((2 * GH + 255) / 256, n), dim3(256), 0, as_stream(stream), j);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

DL4SS_API int dl4ss_birnn_bias_reduce(int cell, int B, int H, int n, void* const* workspaces, float* const* db_ih,
                                      float* const* db_hh, void* stream) {
  return dl4ss_birnn_bias_reduce_ex(cell, B, H, n, workspaces, db_ih, db_hh, 1.f, stream);
}

