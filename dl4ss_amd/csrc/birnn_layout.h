// The recurrence kernels' memory layouts, written once for both sides: the dynamic-LDS regions of
// each of the four persistent kernels (what the kernel carves its pointers from and what the host
// asks the launch for) and the geometry of the hand-off workspace (what the kernels index, the
// launchers zero and dl4ss_birnn_workspace_bytes reports).  Offsets are in floats from the start of
// the dynamic LDS unless a name says bytes; a region's internals (strides within a record, bank-quad
// pads) stay with the kernel that owns it.
#pragma once
#include <hip/hip_runtime.h>

namespace dl4ss_rnn {

#define RNN_HD __host__ __device__ constexpr

constexpr int NT = 512;      // threads per workgroup
constexpr int NROLE = 256;   // generic kernels: [0,256) cell + publish ; [256,512) gather
constexpr int JMAX = 20;     // hidden units per workgroup (the planner's largest J)
constexpr int WMAX = 64;     // fwd weights per thread (generic fp32 path)
constexpr int RPLMAX = 20;   // bwd rows per thread
constexpr int KGLMAX = 6;    // bwd k per thread
constexpr int HMAX = 320;    // largest hidden size of the training kernels (sizes per-thread offset arrays)
constexpr int HMAX_L = 640;  // largest hidden size of the generic kernels' large-H instantiations (forward and
                             // BPTT): the H = 600 speaker classifier of EvalVer.py:305-326 / GRID.py:178-199
constexpr int LDS_BYTES = 160 * 1024;  // a workgroup's LDS on gfx950

// bf16 row strides of the MFMA B images (8 bf16 of pad: rows on distinct bank quads)
RNN_HD int shb_stride(int hm) { return hm / 32 * 32 + 8; }  // forward h image, k < HM (k >= H stays zero)
constexpr int SDG = (4 * JMAX + 31) / 32 * 32 + 8;           // BPTT dgh image, gate rows r < 4 J (rows >= R stay zero)
RNN_HD int mfma_tiles(int R) { return (R + 15) / 16; }      // MT: 16-row W_hh tiles of a workgroup's R gate rows
RNN_HD int bwd_wspan(int hm) { return (hm / 16 + 3) / 4 * 16; }  // BPTT: output units per MFMA wave (4 waves)
RNN_HD int round4(int n) { return (n + 3) & ~3; }

// ---- generic forward (rnn_fwd_kernel)
//   fp32: sh [BC][HP] | spart [KP][BC][R] | sin [2][BC*J][4]
//   MFMA: shb bf16 [16][SHB] | sgate [BC][MT*16] | sin [2][BC*J][4]
// Each region's length in floats: a kernel advances its pointer by the regions before it, in this
// order, and the launch asks for their sum.  Note: a kernel takes from here every length that is a
// compile-time value in its instantiation; a length with run-time arguments (J, R, NG, HP, KP, RP,
// KW) it spells out at the pointer, with this header's name beside it.  Passed through these
// functions -- or through a struct of offsets computed up front -- the same arithmetic reaches the
// optimiser in another order and changed the register allocation of most instantiations
// (tools/kernel_diff.py), which a refactor must not.
RNN_HD int fwd_sh_n(int BC, int HP) { return BC * HP; }
RNN_HD int fwd_spart_n(int KP, int BC, int R) { return KP * BC * R; }
RNN_HD int fwd_shb_n(int hm) { return 8 * shb_stride(hm); }  // 16 rows of bf16
RNN_HD int fwd_sgate_n(int BC, int R) { return BC * mfma_tiles(R) * 16; }
RNN_HD int fwd_sin_n(int BC, int J) { return 2 * BC * J * 4; }
RNN_HD size_t fwd_lds_bytes(bool mf, int hm, int BC, int J, int R, int HP, int KP) {
  return sizeof(float) * (size_t)((mf ? fwd_shb_n(hm) + fwd_sgate_n(BC, R) : fwd_sh_n(BC, HP) + fwd_spart_n(KP, BC, R)) +
                                  fwd_sin_n(BC, J));
}

// ---- generic BPTT (rnn_bwd_kernel)
//   fp32: sdg [BC][RPAD] | sdh [NG][BC][J] | spart [RP][BC][KW] | sop [2][BC*J][8]
//   MFMA: sdgb bf16 [16][SDG] | sdh [NG][BC][J] | spart [4 waves][BC][WSPAN] | sop [2][BC*J][8]
// sdh is rounded up to a float4; the allocation counts 3 floats for that whatever the remainder
// (up to 3 floats of slack behind sop).
RNN_HD int bwd_sdg_n(bool mf, int BC, int RPAD) { return mf ? 8 * SDG : BC * RPAD; }
RNN_HD int bwd_sdh_n(int NG, int BC, int J) { return round4(NG * BC * J); }
RNN_HD int bwd_spart_n(bool mf, int hm, int BC, int RP, int KW) { return mf ? 4 * BC * bwd_wspan(hm) : RP * BC * KW; }
RNN_HD int bwd_sop_n(int BC, int J) { return 2 * BC * J * 8; }
RNN_HD size_t bwd_lds_bytes(bool mf, int hm, int BC, int J, int NG, int RP, int RPAD, int KW) {
  return sizeof(float) * (size_t)(bwd_sdg_n(mf, BC, RPAD) + (NG * BC * J + 3) + bwd_spart_n(mf, hm, BC, RP, KW) + bwd_sop_n(BC, J));
}

// ---- packed forward (rnn_fwd_pk_kernel), HM = HMAX
//   shb bf16 [16][SHB] | sgate [BC][SGS] | sgx [BC][16] | sin [NSIN][sin_slab] | spub bf16 [BC][PKU]
//   fused projection only: | up to 256 B to the next 256-B boundary | ring bf16 [3 SPB][xw_slot]
// spub was the LDS stage of the publish (now DPP wave shifts): unused, kept so that the ring stays
// where it is.
constexpr int PKU = 24;               // staged h slots per (row, producer): 8 granules x 3
constexpr int XKMAX = 2 * HMAX / 32;  // fused input projection: k-steps of 32 (Kin <= 2 HMAX)
// bf16 row stride of its B images: 80 16-B chunks of data + 2 pad chunks (656 bf16 = 328 dwords:
// the BC rows and the zero row land on distinct bank quads for every 16-lane ds_read_b128
// group; at 80 chunks every row started on bank 0, a 4-way conflict, tools/lds_banks.py)
constexpr int SXC = XKMAX * 4 + 2;    // 16-B chunks per row
constexpr int SXB = SXC * 8;
// Fused projection in blocks: one MFMA's 16 B-columns are SPB = 16 / BC consecutive steps x BC
// batch rows, so a tile's projection of a whole block of SPB steps is ONE XK-long MFMA chain
// (a quarter of a per-step form's MFMAs at BC = 4); the chain of block k+1 is split into SPB
// parts, one per step of block k.  The layer-input rows sit in a ring of 3 blocks of step slots
// (slot stride XBUF + 16 BC bf16: the 16 columns' rows on distinct bank quads,
// tools/lds_banks.py), DMA'd two blocks ahead of use.
RNN_HD int xw_spb(int bc) { return 16 / bc; }
// Packed forward's per-step input projections, one slab per step slot: [cell = b * J + u][4 gates],
// read by each cell lane as ONE float4; slab stride BC * 128 + 4 floats (= 4 mod 8).  The fused
// projection's block epilogue (xfinal) stores one gate of 16 (step, batch row) columns per
// instruction: with [b * 32 + u][4] records in 512-float slabs all 16 hit ONE bank (a 16-way
// conflict, ~150 conflict cycles per step and workgroup, SQ_LDS_BANK_CONFLICT / IDX_ACTIVE of the
// fused kernels 0.32 / 0.35); dense rows and the odd quad in the slab stride spread them over 8
// banks (tools/lds_banks.py: 600 -> 104 conflict cycles per block).  A gate-major layout (one
// 16-B epilogue store per lane, conflict-free) measured slower: the cell lanes' 4 scalar reads
// instead of one float4 cost the 600-wide layers 9-17 us per launch (round 4)
RNN_HD int sin_slab(int bc) { return bc * 32 * 4 + 4; }
RNN_HD int xw_nxq(int bc) { return (bc * SXC + 127) / 128; }
RNN_HD int xw_slot(int bc) { return xw_nxq(bc) * 128 * 8 + 16 * bc; }  // bf16
RNN_HD int xw_ring_bf16(int bc) { return 3 * xw_spb(bc) * xw_slot(bc); }
RNN_HD int fwd_pk_nsin(int bc, bool xw) { return xw ? 2 * xw_spb(bc) : 2; }  // double buffered, or two blocks of SPB steps
RNN_HD int fwd_pk_sgs(int R) { return mfma_tiles(R) * 16 + 4; }  // sgate row stride (floats): 4 batch rows on 4 distinct bank quads
RNN_HD int fwd_pk_sgate_n(int BC, int R) { return BC * fwd_pk_sgs(R); }
RNN_HD int fwd_pk_sgx_n(int BC) { return BC * 16; }
RNN_HD int fwd_pk_sin_n(int BC, bool xw) { return fwd_pk_nsin(BC, xw) * sin_slab(BC); }
RNN_HD int fwd_pk_spub_bf16(int BC) { return BC * PKU; }
RNN_HD size_t fwd_pk_lds_bytes(int BC, int R, bool xw) {
  return sizeof(float) * (size_t)(fwd_shb_n(HMAX) + fwd_pk_sgate_n(BC, R) + fwd_pk_sgx_n(BC) + fwd_pk_sin_n(BC, xw)) +
         sizeof(unsigned short) * (size_t)fwd_pk_spub_bf16(BC) +
         (xw ? 256 + sizeof(unsigned short) * (size_t)xw_ring_bf16(BC) : 0);
}

// ---- packed BPTT (rnn_bwd_pk_kernel), HM = HMAX
//   sdgb bf16 [16][SDG] | sdh [16][BC][J] | wsc [4 waves][BC][WSP] | sop [2 steps][2 planes][SOPP] |
//   sraw [2 prefetch waves][7][CPWP]  (the LSTM stages 7 operand slots per cell, the GRU 6: one
//   slot row per wave of slack there; unused at BC <= 2)
constexpr int BWD_PK_WSP = bwd_wspan(HMAX) + 4;  // transpose row stride (floats): rows on distinct bank quads
RNN_HD int bwd_pk_sopp(int bc) { return bc * 32 * 4 + 16; }      // one plane of the per-step operand record
RNN_HD int bwd_pk_cpwp(int bc) { return (bc * JMAX + 1) / 2; }  // raw staging pitch: cells per prefetch wave at J <= 20
RNN_HD int bwd_pk_sdh_n(int BC, int J) { return round4(16 * BC * J); }
RNN_HD int bwd_pk_wsc_n(int BC) { return 4 * BC * BWD_PK_WSP; }
RNN_HD int bwd_pk_sop_n(int BC) { return 2 * 2 * bwd_pk_sopp(BC); }
RNN_HD int bwd_pk_sraw_n(int BC) { return 2 * 7 * bwd_pk_cpwp(BC); }
RNN_HD size_t bwd_pk_lds_bytes(int BC, int J) {
  return sizeof(float) * (size_t)(8 * SDG + bwd_pk_sdh_n(BC, J) + bwd_pk_wsc_n(BC) + bwd_pk_sop_n(BC) + bwd_pk_sraw_n(BC));
}

// ---- hand-off workspace: per group (direction, batch chunk) a block of copies of 8-B granules.
//   generic forward  [2 slots][BC][H]                      generic BPTT  [2 slots][NG][BC][H]
//   packed forward   [2 slots][hand-off, spare][BC][NG][8]  packed BPTT   [2 slots][hand-off, spare][NG][BC][HG]
// The packed kernels' slot s hand-off copy is copy 2 s; the spare copy of slot 1 (copy 3) holds the
// group's placement granules.  Behind the largest of the four areas, 256-B aligned, sit the 256 B of
// the packed kernels' group-formation counters (group_pk), then the BPTT's bias partials.
constexpr int GEN_NCOPY = 2, PK_NCOPY = 4, PK_PLACE_COPY = 3;
constexpr int CTL_BYTES = 256;
RNN_HD int pk_hg(int H) { return ((H + 1) / 2 + 1) & ~1; }  // packed BPTT granules per (producer, row), even: 16-B aligned rows
// granules of n copies (generic kernels: 64-bit throughout, the factors in the kernels' order) / of one
// copy (packed kernels)
RNN_HD long long fwd_copies_g(long long n, int BC, int H) { return n * BC * H; }
RNN_HD int fwd_pk_copy_g(int BC, int NG) { return BC * NG * 8; }
RNN_HD long long bwd_copies_g(long long n, int BC, int NG, int H) { return n * NG * BC * H; }
RNN_HD int bwd_pk_copy_g(int BC, int NG, int H) { return NG * BC * pk_hg(H); }
// bytes of a kernel's granule area (what its launcher zeroes): groups x ncopy x copy_g granules
RNN_HD long long granule_bytes(long long groups, int ncopy, long long copy_g) { return groups * ncopy * copy_g * 8; }
RNN_HD long long max2(long long a, long long b) { return a > b ? a : b; }
// hand-off area of a plan, 256-B aligned; big (H > HMAX): generic kernels only, no counters
RNN_HD long long handoff_area_bytes(long long groups, int BC, int NG, int H, bool big) {
  long long n = max2(granule_bytes(groups, GEN_NCOPY, fwd_copies_g(1, BC, H)), granule_bytes(groups, GEN_NCOPY, bwd_copies_g(1, BC, NG, H)));
  if (!big)
    n = max2(n, max2(granule_bytes(groups, PK_NCOPY, fwd_pk_copy_g(BC, NG)), granule_bytes(groups, PK_NCOPY, bwd_pk_copy_g(BC, NG, H))));
  return (n + 255) / 256 * 256 + (big ? 0 : CTL_BYTES);
}
RNN_HD long long ctl_offset_bytes(long long groups, int BC, int NG, int H) {
  return handoff_area_bytes(groups, BC, NG, H, false) - CTL_BYTES;
}

// ---- the worst case of every kernel fits a workgroup's LDS: J = 20 with the LSTM's R = 80 gate
// rows, every instantiated batch chunk, the fused projection (its ring is sized for XKMAX whatever
// the layer's width), the generic kernels at HM = HMAX_L with NG = 32 workgroups per group.  The fp32
// paths at the planner's bounds: KP = NT / R = 6 k-parts of HP < HMAX_L + 4 KP; RP = 16 row parts of
// RPLMAX rows, KG = NT / RP k-groups of KGLMAX (RP KW <= NT KGLMAX for every RP).
RNN_HD bool lds_fits_all_bc(int which) {
  constexpr int R = 4 * JMAX, NG = HMAX_L / JMAX;
  for (int bc = 1; bc <= 8; bc *= 2) {
    const size_t n = which == 0   ? fwd_pk_lds_bytes(bc, R, true)
                     : which == 1 ? bwd_pk_lds_bytes(bc, JMAX)
                     : which == 2 ? fwd_lds_bytes(true, HMAX_L, bc, JMAX, R, 0, 0)
                     : which == 3 ? fwd_lds_bytes(false, HMAX_L, bc, JMAX, R, HMAX_L + 4 * (NT / R), NT / R)
                     : which == 4 ? bwd_lds_bytes(true, HMAX_L, bc, JMAX, NG, 0, 0, 0)
                                  : bwd_lds_bytes(false, HMAX_L, bc, JMAX, NG, 16, 16 * RPLMAX, NT / 16 * KGLMAX);
    if (n > (size_t)LDS_BYTES) return false;
  }
  return true;
}
static_assert(lds_fits_all_bc(0), "packed forward with the fused projection: LDS");
static_assert(lds_fits_all_bc(1), "packed BPTT: LDS");
static_assert(lds_fits_all_bc(2) && lds_fits_all_bc(3), "generic forward at HMAX_L: LDS");
static_assert(lds_fits_all_bc(4) && lds_fits_all_bc(5), "generic BPTT at HMAX_L: LDS");

#undef RNN_HD

}  // namespace dl4ss_rnn
