// Persistent bidirectional LSTM / GRU recurrence (forward and BPTT) for gfx950.
//
// Replaces the cuDNN recurrence of nn.LSTM(129, 300, 4, bidirectional) at
// TDAA_beta/main_run_sstune_EvalVer.py:282-293 and nn.GRU(129, 300, 2,
// bidirectional) at Torch_multi/main_run.py:263-273 / cRM_EvalVer.py:345-355
// (torch cell equations, gate order i,f,g,o / r,z,n, zero initial state).  The
// input projection X W_ih^T + b_ih is a separate MFMA GEMM (gemm.hip); this
// kernel runs the T dependent steps of one layer, both directions at once.
//
// Decomposition: the batch is cut into chunks of BC utterances; each
// (direction, chunk) is a GROUP of NG workgroups, and workgroup w of a group
// owns J hidden units (all NGATE gates of them: the four LSTM gates are fused
// into ONE matvec per direction per step, so the cell update is local).  Its
// W_hh block (NGATE*J rows x H) lives in REGISTERS for the whole launch; the
// previous hidden state is staged in LDS each step.  Only h (forward) or the
// dh partial sums (backward) cross workgroups, once per step, inside the group.
//
// Hand-off (MI355X_MICROARCH.md, Valid forms / R2 granules): every exchanged
// value is an 8-byte {tag = step+1, fp32 bits} granule written by ONE agent-
// scope relaxed atomic store (global_store sc1) and read by agent-scope
// relaxed loads (sc1) until every tag matches -- no fences, no counter.  Two
// slots alternate by step parity (a slot is rewritten only after every reader
// has consumed it, because producing step s+2 needs all of step s+1).  All
// spins are bounded: a timeout sets *status and the workgroup exits.
// Granule buffers are zeroed by hipMemsetAsync in the launch function.
//
// Wave roles (512 threads = 8 waves, 2 per SIMD): a wave's vmcnt retires
// loads and stores in issue order, so a wave that polls granules must not
// carry outstanding stores.  Waves 0-3 do the cell update and ALL global
// stores (granules first, then prefetch loads for the next step, then the
// saved activations); waves 4-7 only poll granules into LDS.  All 8 waves run
// the register-resident matvec (two waves per SIMD keep the VALU issuing).
// The packed bf16 kernels (rnn_fwd_pk_kernel / rnn_bwd_pk_kernel) split the roles
// differently: waves 0-3 cell + stores, FWD_NPW / BWD_NPW polling waves from wave 4 (the
// forward's second one is wave 7), the rest MFMA tiles + prefetch (see their comments).
// Co-residency: every workgroup of a launch must be resident at once; the plan keeps the
// grid within the device's CUs minus 1/16 (240 on a full MI355X, wg_limit) and every launch
// re-checks it against CUs x occupancy (launch_resident).
//
// Files: this header (kernel arguments, hand-off and prefetch helpers, the co-residency guard) and
// birnn_layout.h (LDS and workspace layouts) are shared; each kernel sits in a file of its own
// with its launch selection -- birnn_fwd.hip / birnn_bwd.hip (generic: fp32 parity mode, one-value
// granules, large H), birnn_fwd_pk.hip / birnn_bwd_pk.hip (packed bf16: the training step);
// birnn.hip holds the planner and the C ABI.
#pragma once
#include <mutex>
#include <type_traits>
#include "birnn_layout.h"
#include "common.h"

namespace dl4ss_rnn __attribute__((visibility("hidden"))) {

enum { CELL_LSTM = DL4SS_CELL_LSTM, CELL_GRU = DL4SS_CELL_GRU };

typedef unsigned long long u64;

// Diagnostic build only (-DRNN_STAMPS, tools/build_stamps.py): per-phase s_memtime
// sums for threads 0 (cell/publish role) and 256 (gather role) of every workgroup.
#ifdef RNN_STAMPS
__device__ __forceinline__ u64 stamp_now() {
  u64 t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define STAMP_DECL u64 st_prev = stamp_now(), st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define STAMP(i) { const u64 n_ = stamp_now(); st_acc[i] += n_ - st_prev; st_prev = n_; }
#ifndef STAMP_T2
#define STAMP_T2 NROLE  // the second recorded thread (320: the first prefetch wave of the packed forward)
#endif
#define STAMP_FLUSH                                                                   \
  if (a.stamps && (threadIdx.x == 0 || threadIdx.x == STAMP_T2))                     \
    for (int i_ = 0; i_ < 8; ++i_) a.stamps[blockIdx.x * 16 + (threadIdx.x ? 8 : 0) + i_] = st_acc[i_];
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH
#endif
// Diagnostic build only (-DRNN_TRACE): per (workgroup, step) s_memrealtime (100 MHz, chip-wide)
// of the publish (slot 0) and of the completed poll (slot 1) in a.stamps[(bid * T + s) * 2 + slot].
#ifdef RNN_TRACE
__device__ __forceinline__ u64 rtc_now() {
  u64 t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define TRACE(slot, s) do { if (a.stamps && (threadIdx.x & 63) == 0) a.stamps[((long long)blockIdx.x * a.T + (s)) * 4 + (slot)] = rtc_now(); } while (0)
#else
#define TRACE(slot, s) do { } while (0)
#endif

// Gate nonlinearities on the serial critical path: v_exp + v_rcp (1 ulp) instead of
// the IEEE division / ocml tanh sequences (the cell update runs on one wave).
__device__ __forceinline__ float fsig(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// tanh(x) = 2 / (1 + 2^(x (-2 log2 e))) - 1: the constant folded into ONE multiply (-2 log2e is exact in
// fp32, so x * (-2 L) rounds the same product as (-2 x) * L did -- bitwise the two-multiply form, one
// dependent VALU op shorter on the recurrences' critical cell chain)
__device__ __forceinline__ float ftanh(float x) {
  return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -2.88539008177792681472f)) - 1.0f;
}

// Keras 1's inner_activation (Theano's hard_sigmoid: slope 0.2, shift 0.5, clip to [0, 1]) of the
// hard-gates LSTM cell: one FMA whose result is clamped (the `clamp` output modifier, no compare chain)
__device__ __forceinline__ float hsig(float x) { return fminf(fmaxf(fmaf(0.2f, x, 0.5f), 0.0f), 1.0f); }
// its derivative from the saved activation s = hsig(x), as the logistic form takes s (1 - s): 0.2 strictly
// inside the clip, 0 on it
__device__ __forceinline__ float hsig_grad(float s) { return (s > 0.0f && s < 1.0f) ? 0.2f : 0.0f; }

typedef short bf16x8 __attribute__((ext_vector_type(8)));

// Sum of the NG producers' dh partials p[i * stride] (BPTT cell phase): for NG <= 16 all
// loads are issued at once and added as a pairwise tree.  (A runtime-bound loop compiled to
// an 8-wide unrolled body plus a remainder loop with one LDS round trip per iteration:
// ~800 of the cell phase's ~1500 cycles per step at NG = 15.)
__device__ __forceinline__ float sum_partials(const float* p, int stride, int NG) {
  if (NG > 16) {
    float a = 0.0f;
    for (int i = 0; i < NG; ++i) a += p[i * stride];
    return a;
  }
  // branch-free: 16 loads from valid addresses (index clamped to NG - 1), then a select --
  // a guarded load per element compiled to a branch and a saved exec mask each
  float v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float x = p[(i < NG ? i : NG - 1) * stride];
    v[i] = i < NG ? x : 0.0f;
  }
#pragma unroll
  for (int w = 8; w > 0; w >>= 1)
#pragma unroll
    for (int i = 0; i < w; ++i) v[i] += v[i + w];
  return v[0];
}
// Sum of 16 producers' dh partials p[i * stride] for the packed BPTT, whose partial buffer
// always holds 16 producer rows (rows >= NG stay zero): no index clamp, no select.  Same
// pairwise tree as sum_partials, so the result is bitwise the same.
__device__ __forceinline__ float sum_partials16(const float* p, int stride) {
  float v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = p[i * stride];
#pragma unroll
  for (int w = 8; w > 0; w >>= 1)
#pragma unroll
    for (int i = 0; i < w; ++i) v[i] += v[i + w];
  return v[0];
}
// Sum of N slot partials p[i * stride], i < N, as a fixed pairwise tree over the next power of two
// (missing leaves are zero): deterministic, and for N = 16 the tree of sum_partials16.
template <int N>
__device__ __forceinline__ float sum_slots(const float* p, int stride) {
  constexpr int P2 = N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : 16;
  static_assert(N >= 1 && N <= 16, "1..16 slots");
  float v[P2];
#pragma unroll
  for (int i = 0; i < P2; ++i) v[i] = i < N ? p[i * stride] : 0.0f;
#pragma unroll
  for (int w = P2 / 2; w > 0; w >>= 1)
#pragma unroll
    for (int i = 0; i < w; ++i) v[i] += v[i + w];
  return v[0];
}
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned short bf16_rne(float f) {
  unsigned u = __float_as_uint(f);
  u += 0x7FFF + ((u >> 16) & 1);
  return (unsigned short)(u >> 16);
}
// The weights are rounded with the same plain RNE when a launch loads its W_hh fragments.  No NaN
// special case here: values formed by arithmetic are canonical quiet NaNs (0x7FC00000 / 0xFFC00000),
// which round to NaN, and the NaN-preserving form (bf16_bits_rne) in the once-per-launch weight
// loads changed the packed kernels' code generation enough to cost 4.3 % of the step (A/B, 20 steps
// x 2 alternating runs: 7768 / 7776 vs 8109 / 8097 mixtures/s, round 4).

__device__ __forceinline__ void put_granule(u64* g, unsigned tag, float v) {
  const u64 x = ((u64)tag << 32) | (u64)__float_as_uint(v);
  __hip_atomic_store(g, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 get_granule(const u64* g) {
  return __hip_atomic_load(const_cast<u64*>(g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct RnnArgs {
  int B, T, H, J, NG, nchunk;
  int KP, KPL, HP;       // fwd: k-parts, k per part (mult of 4), padded H
  int RP, RPL, KG, KGL;  // bwd: row parts, rows per part, k groups, k per group
  const float* G;        // fwd (B,T,2,NGATE*H) input projections (+ b_ih)
  const float* Whh;      // (2, NGATE*H, H)
  const float* bhh;      // (2, NGATE*H)
  float* out;            // (B,T,2H) layer output h
  float* hprev;          // (B,T,2H) h_{t-1} per step (zero at the sequence start)
  float* act;            // (B,T,2,4H) LSTM: i,f,g,o ; GRU: r,z,n,(W_hn h + b_hn)
  float* cs;             // (B,T,2,H) LSTM cell states
  const float* dOut;     // bwd (B,T,2H), or dout_ns split-K slabs of it dout_zs floats apart (summed in order)
  int dout_ns;
  long long dout_zs;
  const float* dOutB;    // bwd optional (B,2H) added to dOut at every t (d mean_t h)
  float* dG;             // bwd (B,T,2,NGATE*H) grad wrt input projection (pre-activation)
  float* dGh;            // bwd GRU: grad wrt W_hh h + b_hh (LSTM: == dG, may be null)
  u64* xbuf;             // granules
  int* status;
  unsigned spin_limit;   // polls before a hand-off times out (SPIN_LIMIT; dl4ss_debug_set_spin_limit)
  int place_force;       // packed kernels: 1 = write-through hand-off regardless of placement (test hook)
  u64* stamps;           // diagnostic build only
  // bf16 mode extras (packed kernels only; any may be null)
  unsigned short* outb;    // fwd (B,T,2H) bf16(h)          -- next layer's / Linear's GEMM operand
  unsigned short* hprevb;  // fwd (B,T,2H) bf16(h_{t-1})    -- dW_hh GEMM operand
  unsigned short* dGb;     // bwd (B,T,2,NGATE*H) bf16(dG)  -- dW_ih / dX GEMM operand
  unsigned short* dGhb;    // bwd GRU: bf16(dGh)            -- dW_hh GEMM operand
  int ghb;                 // bwd GRU: dGhb's per-direction column stride (NGATE*H, or padded to a
                           //      multiple of 8 by DL4SS_RNN_DGH_PAD8: 16-B aligned GEMM operand rows)
  float* dbi;              // bwd: += sum_{b,t} dG   (bias_ih gradient, (2, NGATE*H))
  float* dbh;              // bwd: += sum_{b,t} dGh  (bias_hh gradient)
  float* dbpart;           // bwd: per-row bias sums [b][d][ih | hh][NGATE*H] (fixed-order reduce), or
                           //      null: float atomics straight into dbi / dbh
  // fused input projection (packed forward, rnn_fwd_pk_kernel<.., true>): G is not read; each
  // step's x_t W_ih^T + b_ih is formed in the kernel from the bf16 layer input
  const unsigned short* Xb;    // (B*T, ldx) bf16 layer input rows, k < Kin (padding never read)
  const unsigned short* Wihb;  // (2*NGATE*H, ldw) bf16 W_ih rows (direction-major), k < Kin
  const float* bih;            // (2, NGATE*H)
  int Kin;
  long long ldx, ldw;
  // act layout: 0 gate-major (B,T,2,4H); 1 cell-major (B,T,2,H,4) -- the packed kernels at BC >= 4
  // (act_cell_major): the forward stores a cell's four gates as one 16-B store, the BPTT loads them
  // as one 16-B item
  int act_cm;
  float* hmean;  // fwd (packed): (B, 2H) mean over t of h, summed by each cell lane in step order (or null)
  unsigned* gctl;  // packed kernels: the group-formation counters (zeroed with the workspace; group_pk)
};

__device__ __forceinline__ void group_of(int bid, int NG, int ngroups, int& group, int& w) {
  if ((ngroups & 7) == 0) {  // keep a group's workgroups on one XCD (speed only: bid % 8 share an XCD)
    const int x = bid & 7, y = bid >> 3;
    group = x * (ngroups >> 3) + y / NG;
    w = y % NG;
  } else {
    group = bid / NG;
    w = bid % NG;
  }
}

// Per-timestep operand prefetch, run by the gather waves so that the cell waves
// issue no loads at all (their vmcnt then only ever holds stores): item q is
// p[q][(t + shift[q]) * stride[q]] (0 outside [0, T)), landing in LDS at dst[q].
// Loads for step s+1 are issued during step s and committed to LDS at step s+1
// (by then the granule poll has already waited past them).
// NZ > 1 (the BPTT's dOut, DL4SS_RNN_DOUT_SLABS): an item with zq[q] set is the sum of NZ split-K
// slabs zs floats apart, all loaded at issue and added at commit in slab order from zero -- bitwise the
// gemm_gl split-K combine it replaces (((0 + s0) + s1) + ...).  NZ is the launch's exact slab count (a
// kernel template argument): a runtime count per item (round 6's first form, NZ = 4 in every launch)
// cost ~20 us per BPTT launch even at one slab (profiles/r06_nz_ab.txt).
template <int NQ, int NZ = 1>
struct StepLoader {
  const float* p[NQ];
  int stride[NQ], shift[NQ], dst[NQ];
  float v[NQ];
  bool zq[NQ];
  long long zs;
  float vz[NQ][NZ > 1 ? NZ - 1 : 1];
  __device__ __forceinline__ void issue(int t, int T) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int tt = t + shift[q];
      const bool ok = p[q] != nullptr && tt >= 0 && tt < T;
      v[q] = ok ? p[q][(long long)tt * stride[q]] : 0.0f;
      if constexpr (NZ > 1) {
#pragma unroll
        for (int z = 1; z < NZ; ++z)
          vz[q][z - 1] = (ok && zq[q]) ? p[q][(long long)tt * stride[q] + z * zs] : 0.0f;
      }
    }
  }
  __device__ __forceinline__ void commit(float* lds) const {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (dst[q] < 0) continue;
      float x = v[q];
      if constexpr (NZ > 1) {
        if (zq[q]) {
          x = 0.0f + v[q];
#pragma unroll
          for (int z = 1; z < NZ; ++z) x += vz[q][z - 1];
        }
      }
      lds[dst[q]] = x;
    }
  }
};


// Poll the granules src[off[g]] (off < 0: nothing to read) until every tag == tag;
// returns false on timeout.  Offsets are computed once per launch by the caller;
// all loads of the thread are in flight at once and only stale ones are re-issued.
template <int GM>
__device__ __forceinline__ bool gather(const u64* src, const int (&off)[GM], unsigned tag, u64 (&v)[GM],
                                       unsigned limit) {
  const u64 done = (u64)tag << 32;
#pragma unroll
  for (int g = 0; g < GM; ++g) v[g] = off[g] >= 0 ? get_granule(src + off[g]) : done;
  unsigned spins = 0;
  while (true) {
    bool ok = true;
#pragma unroll
    for (int g = 0; g < GM; ++g) ok &= (unsigned)(v[g] >> 32) == tag;
    if (ok) return true;
    if (++spins > limit) return false;
    __builtin_amdgcn_s_sleep(1);
#pragma unroll
    for (int g = 0; g < GM; ++g)
      if ((unsigned)(v[g] >> 32) != tag) v[g] = get_granule(src + off[g]);
  }
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int WPOLL = 4;    // the polling wave (BPTT: the first of BWD_NPW)
constexpr int BWD_NPW = 2;  // BPTT polling waves
constexpr int FWD_MV_CHAINS = 2;  // forward bf16 matvec: accumulator chains per MFMA tile (4: 367 vs 363 us per pass)
constexpr int FWD_NPW = 2;  // forward polling waves: 4, and 7 when >= 2, and 6 when 3 (their MFMA tile indices must be >= MT)
static_assert(FWD_MV_CHAINS >= 1 && FWD_MV_CHAINS <= 8, "FWD_MV_CHAINS: 1..KSMAX accumulator chains");
static_assert(FWD_NPW >= 1 && FWD_NPW <= 3, "FWD_NPW: 1..3 polling waves");
static_assert(BWD_NPW >= 1 && BWD_NPW <= 3, "BWD_NPW: 1..3 polling waves");

__device__ __forceinline__ __amdgpu_buffer_rsrc_t granule_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

__device__ __forceinline__ unsigned xcc_id() {
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  return x & 0xFu;
}

// Group formation of the packed kernels by PLACEMENT, not by block index (round 5).  group_of assumes
// blocks b and b + 8 share an XCD -- true when a launch is dispatched alone, but a kernel dispatched
// concurrently on another stream (the side-stream GEMM, RCCL kernels) interleaves its workgroups into the
// XCD round robin, the groups then span XCDs, and every hand-off of the launch goes write-through and
// cross-XCD: the BPTT ran at twice its time (662 vs 336 us per launch).  Here each workgroup takes a slot
// on a per-XCD counter (device-scope atomic, returning): slot s < cap = NG * ngroups / 8 of XCD x is
// member s % NG of group x * ngroups / 8 + s / NG -- every group on one XCD whatever the dispatch order.
// A workgroup past its XCD's cap waits until every workgroup has taken a slot (the sum of the counters
// reaches the grid: all are co-resident, the plan guarantees it), then takes the ov-th unfilled (group,
// member) in XCD order.  Roles never depend on results, so the arithmetic is bitwise the same.
// ctl: 10 zeroed words (8 per-XCD counters, 1 overflow counter, the release_start count); smem: 2
// words of scratch LDS.
__device__ __forceinline__ void group_pk(unsigned* ctl, int NG, int ngroups, unsigned limit, int* status, float* smem,
                                         int& group, int& w) {
  if (ctl == nullptr || (ngroups & 7) != 0) {
    group_of(blockIdx.x, NG, ngroups, group, w);
    return;
  }
  int* sg = reinterpret_cast<int*>(smem);
  if (threadIdx.x == 0) {
    const int per = ngroups >> 3, cap = per * NG, nwg = ngroups * NG;
    const unsigned x = xcc_id() & 7u;
    const int slot = (int)__hip_atomic_fetch_add(ctl + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int g = -1, m = 0;
    if (slot < cap) {
      g = (int)x * per + slot / NG;
      m = slot % NG;
    } else {
      const int ov = (int)__hip_atomic_fetch_add(ctl + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unsigned c[8];
      unsigned spins = 0;
      while (true) {
        int tot = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          c[i] = __hip_atomic_load(ctl + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          tot += (int)c[i];
        }
        if (tot >= nwg) break;
        if (++spins > limit) {
          atomicOr(status, 8);
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      int k = ov;
      for (int i = 0; i < 8 && g < 0; ++i) {
        const int filled = min((int)c[i], cap), holes = cap - filled;
        if (k < holes) {
          g = i * per + (filled + k) / NG;
          m = (filled + k) % NG;
        }
        k -= holes;
      }
      if (g < 0) group_of(blockIdx.x, NG, ngroups, g, m);  // timed out (status 8): any role, results invalid
    }
    sg[0] = g;
    sg[1] = m;
  }
  __syncthreads();
  group = sg[0];
  w = sg[1];
  __syncthreads();  // the scratch words are reused by the kernel's own LDS
}

// Workspace reuse without a zero fill (round 5).  The packed kernels' hand-off granules need no
// clearing between launches of the same shape: a consumer polls slot (s-1)&1 for tag s at step s
// and a completed launch leaves tags T and T-1 behind, which only steps 1 and 2 could see before
// this launch overwrites them -- never equal for T >= 4 (tags are (step + 1) mod 2^16, T < 65535).
// The group-formation counters and the placement granules {tag 1, XCC id} are what a fill was
// for: the LAST workgroup past the start (all have formed their groups and read the placement by
// then) puts them back to zero.  ctl word 9 counts the workgroups past the start.
// place_stride: u64 between groups' granule blocks; place_off: the placement granules' offset.
__device__ __forceinline__ void release_start(unsigned* ctl, u64* xbuf, int ngroups, int NG, long long place_stride,
                                              long long place_off) {
  if (ctl == nullptr) return;
  // relaxed: this workgroup's reads of the counters and placement granules completed before the
  // startup barrier (their values were used); an acq_rel RMW would write back / invalidate the L2
  const unsigned k = __hip_atomic_fetch_add(ctl + 9, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((int)k != ngroups * NG - 1) return;
  for (int g = 0; g < ngroups; ++g)
    for (int m = 0; m < NG; ++m)
      __hip_atomic_store(xbuf + g * place_stride + place_off + m, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int i = 0; i < 10; ++i) __hip_atomic_store(ctl + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Placement check at launch start (packed kernels).  A group's hand-off granules may be
// written with PLAIN stores only when every workgroup of the group runs on one XCD: a plain
// store stays in that XCD's L2, which serves the peers' `sc1` polls (MI355X_MICROARCH.md,
// stores of each flavour); across XCDs only `sc1` write-through stores are visible.  HIP
// promises no placement (bid % 8 -> XCD is observed, not guaranteed), so every workgroup
// publishes its XCC id as one granule {tag 1, id} and the polling wave gathers the group's NG
// ids.  Every workgroup of the group reads the same NG ids and so picks the same form.
// Called by the polling wave; returns (wave-uniform) true when the granules must be written
// through.  force: 1 = write-through regardless (test hook), 0 = by placement.
__device__ __forceinline__ bool group_needs_write_through(const u64* place, int NG, int lane, unsigned limit,
                                                          int* status, int force) {
  unsigned id = 0;
  bool ok = true;
  if (lane < NG) {
    u64 v = get_granule(place + lane);
    unsigned spins = 0;
    while ((unsigned)(v >> 32) != 1u) {
      if (++spins > limit) {
        ok = false;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      v = get_granule(place + lane);
    }
    id = (unsigned)v;
  }
  if (!ok) atomicOr(status, 4);
  const unsigned id0 = __shfl(id, 0);
  const bool same = !__any(lane < NG && (id != id0 || !ok));
  return force == 1 || !same;
}

// compile-time (rows, k) per thread of the BPTT matvec: the shipped H = 300 plans
// (LSTM R=80: 20 x 3, GRU R=60: 20 x 2) and the generic (guard-free, zero-padded) maxima
// big (H > HMAX): the fp32 plan of the H = 600 LSTM (J = 12: 48 gate rows over 3 parts of 16, 170
// k-groups of 4) and every other wide plan within 16 x 4 run one 16 x 4 instantiation; the rest (the
// H = 600 GRU: J = 17, parts of 17 rows) the runtime-bounds one
inline void bwd_dims(int rpl, int kgl, int& rpln, int& kgln, bool big = false) {
  if (big && rpl <= 16 && kgl <= 4) {
    rpln = 16;
    kgln = 4;
  } else if (!big && ((rpl == 20 && kgl == 3) || (rpl == 20 && kgl == 2))) {
    rpln = rpl;
    kgln = kgl;
  } else {
    rpln = RPLMAX;
    kgln = KGLMAX;
  }
}

// CUs of the current device (cached per device id); 0 when no device is visible
inline int device_cu_count() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cache[dev] == 0) {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cache[dev] = cu;
  }
  return cache[dev];
}

// Launch-time guard of the co-residency assumption: the grid must not exceed the CUs times
// the kernel's occupancy at this LDS size (a persistent launch whose workgroups cannot all
// be resident would spin to the hand-off timeout on every step).
template <typename K>
bool fits_resident(K kernel, int grid, size_t smem) {
  struct Entry { const void* k; size_t smem; int dev; int occ; };
  static std::mutex mu;
  static Entry cache[64];
  static int n = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const void* kp = reinterpret_cast<const void*>(kernel);
  std::lock_guard<std::mutex> lk(mu);
  int occ = -1;
  for (int i = 0; i < n; ++i)
    if (cache[i].k == kp && cache[i].smem == smem && cache[i].dev == dev) occ = cache[i].occ;
  if (occ < 0) {
    occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, NT, smem) != hipSuccess) occ = 0;
    if (n < 64) cache[n++] = Entry{kp, smem, dev, occ};
  }
  return grid <= occ * device_cu_count();
}

// every persistent recurrence launch goes through the co-residency guard
template <typename K>
int launch_resident(K kernel, int grid, size_t smem, hipStream_t st, const RnnArgs& a) {
  if (!fits_resident(kernel, grid, smem)) return (int)hipErrorCooperativeLaunchTooLarge;
  RnnArgs arg = a;
  void* args[] = {&arg};
  return (int)hipLaunchKernel(reinterpret_cast<const void*>(kernel), dim3(grid), dim3(NT), args, smem, st);
}

// The kernel files' entries: each picks its kernel's instantiation for (cell, BC, the plan in a) and
// launches it through launch_resident; hipErrorInvalidValue for a BC that is not instantiated.
// mf: the bf16 MFMA matvec (else the fp32 VALU one).  hard: Keras 1's hard_sigmoid gates (fp32 LSTM only; the
// runtime-bounds instantiations, so the BPTT's LDS is sized for bwd_dims' generic maxima).
// RNN_EXP_MINIMAL (experiment variant libraries only, tools/variant_lib.py --minimal): only the packed
// bf16 kernels at BC = 4 are instantiated -- the C2 / C4 training step at B = 32 -- so a variant of a
// packed-kernel file compiles in a fraction of the full build's time; every other plan fails its launch.
int launch_fwd(const RnnArgs& a, int cell, int BC, bool mf, bool hard, int grid, size_t smem, hipStream_t st);
int launch_fwd_pk(const RnnArgs& a, int cell, int BC, int grid, size_t smem, hipStream_t st);
int launch_bwd(const RnnArgs& a, int cell, int BC, bool mf, bool hard, int grid, size_t smem, hipStream_t st);
int launch_bwd_pk(const RnnArgs& a, int cell, int BC, int grid, size_t smem, hipStream_t st);

}  // namespace dl4ss_rnn
