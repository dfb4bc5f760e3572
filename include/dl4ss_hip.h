/* dl4ss_hip.h -- C ABI of libdl4ss_hip.so, the MI355X (gfx950) hot path of the
 * DL4SS speech-separation training step.
 *
 * Conventions (every entry point):
 *   - returns int: a hipError_t, 0 = success; never throws, never allocates;
 *   - every buffer is a caller-owned device pointer (fp32 unless stated), with
 *     shapes passed as ints; workspaces are caller-allocated;
 *   - `stream` is a hipStream_t passed as void*; the call is asynchronous on it;
 *   - the only library state is per-kernel constant tables; calls on distinct
 *     streams are thread-safe.
 *
 * The reference (shincling/DL4SS) is Python-2 / torch-0.3 code with no native or
 * plugin interface; each entry point below cites the reference call site whose
 * arithmetic it replaces.  The Python boundary (dl4ss_amd.config / predata_* /
 * myNet / test_multi_labels_speech / bss_test) is what binds them; see
 * INTEGRATION.md.
 */
#ifndef DL4SS_HIP_H
#define DL4SS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- STFT / iSTFT ------------------------------------------------------ */
enum {
  DL4SS_STFT_COMPLEX = 1, /* write X (n_sig, T, F, 2) [re, im]                     */
  DL4SS_STFT_MAG = 2,     /* write |X| (n_sig, T, F)                              */
  DL4SS_STFT_LOGMAG = 4,  /* write log(|X| + 2.22e-16) into `mag` instead         */
  DL4SS_STFT_CONJ = 8     /* librosa <= 0.5.x convention (conjugated spectrum)    */
};

/* Framed STFT, n_fft = 256, hop = 128, periodic Hann, centre / reflect padding;
 * T = 1 + n_samples / 128, F = 129.  x: (n_sig, n_samples).
 * Replaces np.transpose(librosa.core.spectrum.stft(y, 256, 128)) and its abs /
 * log-abs at Torch_multi/predata_multiAims_dB.py:180,194,209,214 and
 * TDAA_beta/predata_fromList_cRM_123.py:215-255 (convert2 layout = [re, im]). */
int dl4ss_stft_fwd(const float* x, long long n_sig, int n_samples, int n_fft, int hop, int flags,
                   float* X_c64, float* mag, void* stream);
/* dl4ss_stft_fwd that also writes bf16 (round-to-nearest-even) copies of the magnitudes (or log
 * magnitudes) of the first n_sig_bf16 signals: mag_bf16[(sig * T + t) * ld_bf16 + f], ld_bf16 >= 129,
 * columns >= 129 untouched -- the bf16 recurrence's first-layer input rows without a conversion pass.
 * mag_bf16 NULL: dl4ss_stft_fwd. */
int dl4ss_stft_fwd_ex(const float* x, long long n_sig, int n_samples, int n_fft, int hop, int flags, float* X_c64,
                      float* mag, void* mag_bf16, long long ld_bf16, long long n_sig_bf16, void* stream);

/* Overlap-add inverse STFT: S (n_sig, T, 129, 2) -> y (n_sig, 128 * (T - 1)).
 * Replaces librosa.core.spectrum.istft(S.T, 128) at
 * TDAA_beta/main_run_sstune_EvalVer.py:64-65 and main_run_sstune_cRM_EvalVer.py:98-99.
 * flags: DL4SS_STFT_CONJ only. */
int dl4ss_istft(const float* S_c64, long long n_sig, int T, int n_fft, int hop, int flags, float* y,
                void* stream);
/* Mask apply + iSTFT in one pass (eval output path): signal s (n_sig of them) is
 * synthesised from mixture s / k_per_mix.  mode 0: aux = masked magnitude (n_sig,T,129)
 * with the mixture phase (EvalVer.py:56-65); mode 1: aux = complex ratio mask
 * (n_sig,T,129,2) times the mixture spectrum (cRM_EvalVer.py:96-99,720-728).
 * conj: the mixture spectrum is stored conjugated (librosa <= 0.5). */
int dl4ss_istft_apply(const float* X_mix_c64, const float* aux, long long n_sig, int k_per_mix, int T, int mode,
                      int conj, float* y, void* stream);

/* ---- R1 preprocessing / mixing ----------------------------------------- */
/* raw (B, K, N) -> out_src (B, K, N): each source x -> (x - mean) / max|x - mean| * gain;
 * out_mix (B, N): their sum.  stats_ws: 32*B*K floats of workspace (16-B aligned; K <= 16).
 * Replaces Torch_multi/predata_multiAims_dB.py:156-197 (and the _3dB /
 * fromList_cRM_123 gain variants: gains are computed by the caller). */
int dl4ss_mix_sources(const float* raw, const float* gains, int B, int K, int N, float* stats_ws, float* out_src,
                      float* out_mix, void* stream);
/* As dl4ss_mix_sources, with per-source valid lengths (B*K int32; NULL = N): mean and peak
 * over the first lengths[s] samples, zero beyond -- a list-file wav shorter than MAX_LEN
 * (TDAA_beta/predata_fromList_cRM_123.py:186-201: crop, normalise, then zero-pad). */
int dl4ss_mix_sources_ex(const float* raw, const int* lengths, const float* gains, int B, int K, int N,
                         float* stats_ws, float* out_src, float* out_mix, void* stream);
/* As dl4ss_mix_sources_ex, plus the train-split augmentation of the list loaders: source s is
 * rotated by shifts[s] (B*K int32; NULL = none; taken modulo the source's length) after the
 * normalisation and before the zero-padding -- np.append(x[s:], x[:s]) over the source's own
 * length (TDAA_beta/predata_fromList.py:150-151, predata_fromList_cRM_123.py:198-200). */
int dl4ss_mix_sources_rot(const float* raw, const int* lengths, const int* shifts, const float* gains, int B, int K,
                          int N, float* stats_ws, float* out_src, float* out_mix, void* stream);

/* ---- dense contractions (MFMA) ------------------------------------------ */
enum { DL4SS_EPI_NONE = 0, DL4SS_EPI_TANH = 1, DL4SS_EPI_TANH_BF16 = 2 /* tanh, C written as bf16 */,
       DL4SS_EPI_SPLIT_SLABS = 3 /* dl4ss_gemm_bf16_gl split-K only: the S fp32 slabs stay in ws
                                    ([S][batch][M][N], S = dl4ss_gemm_bf16_gl_ws_bytes / (batch M N 4)),
                                    no combine, C not written: their consumer sums them (the
                                    BPTT's DL4SS_RNN_DOUT_SLABS) */ };
enum { DL4SS_PREC_F32 = 0, DL4SS_PREC_BF16 = 1 };
/* C = op(A) op(B) (+ bias[N]) (tanh) (+ beta C); row-major, leading dims in elements.
 * transA: A stored K x M (else M x K); transB: B stored N x K (else K x N).
 * splitk > 1: C += op(A) op(B) with fp32 atomics (epilogue none, beta 1).
 * Replaces the cuDNN input projection inside nn.LSTM/nn.GRU (EvalVer.py:282-293),
 * nn.Linear(600, 6450) + tanh (EvalVer.py:290,298-299) and their autograd GEMMs. */
int dl4ss_gemm(int transA, int transB, int M, int N, int K, const float* A, long long lda, const float* B,
               long long ldb, float* C, long long ldc, const float* bias, int epilogue, float beta, int precision,
               int splitk, void* stream);
/* dl4ss_gemm with a fixed-order split-K (fp32 parity mode): no atomics, the same bits on every launch.
 * The k-ranges are dl4ss_gemm's: kps = dl4ss_gemm_fixed_kps(K, splitk) = ceil(ceil(K / splitk) / 16) * 16,
 * S = ceil(K / kps).  Workgroup (tile, z) stores its tile into slab z of ws ([S][M][N] fp32, dense), which is
 * bitwise the unsplit kernel on k-range z; a combine launch then forms
 *   C = ((p_0 + p_1) + ... + p_{S-1}) (+ bias[N]) (+ beta C)
 * in that order (beta applied as one fmaf; C is not read when beta == 0; only columns < N are written).
 * S == 1: exactly dl4ss_gemm's unsplit launch (any epilogue or precision; ws unused).  S > 1: DL4SS_EPI_NONE
 * and DL4SS_PREC_F32 only, any beta, optional bias; ws must hold dl4ss_gemm_fixed_ws_bytes(M, N, K, splitk)
 * bytes (0 when S == 1), hipErrorInvalidValue otherwise. */
int dl4ss_gemm_fixed_kps(int K, int splitk);
long long dl4ss_gemm_fixed_ws_bytes(int M, int N, int K, int splitk);
int dl4ss_gemm_fixed(int transA, int transB, int M, int N, int K, const float* A, long long lda, const float* B,
                     long long ldb, float* C, long long ldc, const float* bias, int epilogue, float beta,
                     int precision, int splitk, void* ws, long long ws_bytes, void* stream);

/* y[i] = bf16(x[i]) (round to nearest even), n elements; x 16-B aligned, y 8-B aligned. */
int dl4ss_f32_to_bf16(const float* x, void* y, long long n, void* stream);
/* bf16-operand GEMM with LDS-DMA staging (gemm_gl.hip): every GEMM of the bf16 step.  A and B
 * are raw bf16 words already rounded by their producers, C fp32 (or bf16 with the tanh-bf16
 * epilogue); layout, bias and epilogue as dl4ss_gemm.  Strided batch: member i uses
 * A + i*strideA, B + i*strideB, C + i*strideC (elements).  Deterministic split-K (fp32
 * slabs in ws, dl4ss_gemm_bf16_gl_ws_bytes bytes, then a fixed-order reduce; EPI_NONE only).
 * Needs lda / ldb / strides % 8 == 0, 16-B aligned A / B, for a k-major operand a row stride
 * >= its row count rounded up to 8, and for a k-contiguous one a row stride >= K rounded up
 * to 8 with zeros in that padding; hipErrorInvalidValue otherwise. */
long long dl4ss_gemm_bf16_gl_ws_bytes(int M, int N, int K, int splitk, int batch);
/* Tuning knob: tile configuration of dl4ss_gemm_bf16_gl (0 = per shape, 1 = 128 x 128 double
 * buffer, 2 = 256 x 128 three stages, 3 = 128 x 128 three stages, 4 / 5 = 256 x 256 ping-pong,
 * 6 / 7 = 128 x 128 with five / four 32-deep k-tile stages). */
int dl4ss_gemm_gl_set_config(int cfg);
int dl4ss_gemm_bf16_gl(int transA, int transB, int M, int N, int K, const void* A, long long lda, const void* B,
                       long long ldb, float* C, long long ldc, const float* bias, int epilogue, float beta,
                       int splitk, int batch, long long strideA, long long strideB, long long strideC, void* ws,
                       long long ws_bytes, void* stream);
/* Grouped form: n <= 16 independent problems C_i = op(A_i) op(B_i) + beta_i C_i (same transA /
 * transB for all, no bias, EPI_NONE, per-problem split-K factor) as ONE GEMM launch plus one
 * split-K combine launch; each C_i bitwise equal to dl4ss_gemm_bf16_gl with the same split factor.
 * The backward's weight gradients (dW_lin, every layer's dW_ih and both directions' dW_hh), which
 * the reference accumulates in loss.backward() (TDAA_beta/main_run_sstune_EvalVer.py:673).  The
 * arrays are host arrays of n entries; ws holds dl4ss_gemm_bf16_gl_grouped_ws_bytes bytes. */
long long dl4ss_gemm_bf16_gl_grouped_ws_bytes(int n, const int* M, const int* N, const int* K, const int* splitk);
int dl4ss_gemm_bf16_gl_grouped(int n, int transA, int transB, const int* M, const int* N, const int* K,
                               const void* const* A, const long long* lda, const void* const* B, const long long* ldb,
                               float* const* C, const long long* ldc, const float* beta, const int* splitk, void* ws,
                               long long ws_bytes, void* stream);
/* The grouped launch in its persistent form: `grid` workgroups walk the tiles (grid <= 0: one per
 * tile); cfg 1 = 128 x 128 double buffer, 2 = 256 x 128 three stages (one workgroup per CU);
 * one_per_cu pads cfg 1's LDS to one workgroup per CU.  For a side stream on the CUs the persistent
 * recurrence leaves free (its co-residency budget, dl4ss_birnn_plan_info).  rowsum (NULL or n
 * entries, each NULL or M_i floats): rowsum_i[m] = beta_i rowsum_i[m] + sum_k op(A_i)(m, k), for
 * unsplit problems whose operands are both k-major (transA, !transB) -- the Linear's bias gradient
 * sum_rows dPre (EvalVer.py:290, loss.backward() at :673) beside dW_lin. */
int dl4ss_gemm_bf16_gl_grouped_ex(int n, int transA, int transB, const int* M, const int* N, const int* K,
                                  const void* const* A, const long long* lda, const void* const* B,
                                  const long long* ldb, float* const* C, const long long* ldc, const float* beta,
                                  const int* splitk, void* ws, long long ws_bytes, int grid, int cfg, int one_per_cu,
                                  float* const* rowsum, void* stream);
/* Split-precision operand image: x = hi + lo (hi = bf16(x), lo = bf16(x - hi)); segment s of each
 * row of y (width segw >= cols, zero-padded; s < nseg <= 8) holds hi, or lo when bit s of pattern
 * is set; zeros up to ldy.  [x_hi | x_lo | x_hi] against weights [w_hi | w_hi | w_lo] makes one bf16
 * GEMM with K' = 3 K fp32-accurate (~2^-16): the split forward GEMMs of the "bf16s" step, whose
 * masked magnitude meets the 1e-3 bar on the BiGRU nets (EvalVer.py:282-299 nn.LSTM / Linear). */
int dl4ss_f32_to_bf16_hilo(const float* x, long long ldx, int rows, int cols, void* y, long long ldy, int segw,
                           int nseg, unsigned pattern, void* stream);
/* 2-D form with row padding: y[r*ldy + c] = bf16(x[r*ldx + c]) (c < cols), 0 up to ldy. */
int dl4ss_f32_to_bf16_2d(const float* x, long long ldx, int rows, int cols, void* y, long long ldy, void* stream);
/* out[n] += sum_m A[m*lda + n] for a bf16 matrix A (bias gradient from bf16 dPre). */
int dl4ss_colsum_bf16(const void* A, long long lda, int M, int N, float* out, void* stream);
/* Deterministic form: per-256-row-block partials in part (dl4ss_colsum_bf16_part_bytes(M, N)
 * bytes), then a fixed-order reduce into out (bitwise reproducible bias gradients). */
long long dl4ss_colsum_bf16_part_bytes(int M, int N);
int dl4ss_colsum_bf16_det(const void* A, long long lda, int M, int N, float* out, float* part, long long part_bytes,
                          void* stream);
/* dl4ss_colsum_bf16_det with out = beta out + sums (beta 0: out written, not read; beta 1 bitwise _det). */
int dl4ss_colsum_bf16_det_ex(const void* A, long long lda, int M, int N, float* out, float* part,
                             long long part_bytes, float beta, void* stream);
/* n (<= 8) dl4ss_f32_to_bf16_2d conversions in one launch (host arrays of per-segment
 * arguments): the step's bf16 weight copies (W_ih of every layer, the Linear). */
int dl4ss_f32_to_bf16_2d_multi(int n, const float* const* x, const long long* ldx, const int* rows, const int* cols,
                               void* const* y, const long long* ldy, void* stream);

/* ---- persistent bidirectional LSTM / GRU recurrence ---------------------- */
enum { DL4SS_CELL_LSTM = 0, DL4SS_CELL_GRU = 1 };
/* Workspace (bytes) needed by dl4ss_birnn_fwd / _bwd for (cell, B, H); -1 if unsupported: the
 * hand-off granules, then (bf16 BPTT with fused bias gradients) the per-row bias partials that
 * a fixed-order reduce adds into db_ih / db_hh, so the gradients are bitwise reproducible.
 * The launchers zero the workspace themselves (hipMemsetAsync) unless `precision` carries
 * DL4SS_RNN_WS_ZEROED: the caller then guarantees it is zero (e.g. one fill per training
 * step over separate workspaces for every layer and pass) -- or exactly as the previous launch
 * on it left it, when that launch had the same (cell, B, T, H), T >= 4, and completed without a
 * timeout: its stale tags cannot match, and the packed kernels reset their start counters and
 * placement granules themselves (the training step zeroes its workspaces once). */
#define DL4SS_RNN_WS_ZEROED 0x100
/* precision flag of dl4ss_birnn_bwd_ex: dGh_bf16 is laid out (B, T, 2, pad8(NGATE*H)) -- each
 * direction's columns start 16-B aligned (the GRU's 900 gate rows -> 904), so both directions'
 * dW_hh run as one LDS-DMA batched GEMM (gemm_gl).  The unpadded default is (B, T, 2, NGATE*H).  The pad
 * columns (900..903 of each direction at H = 300) are NOT written (as the M extent of a k-major gemm_gl
 * operand they never reach a result). */
#define DL4SS_RNN_DGH_PAD8 0x200
/* precision flag of dl4ss_birnn_bwd_ex (bf16 BPTT with fused bias gradients): leave the per-row
 * bias partials in the workspace; dl4ss_birnn_bias_reduce adds those of n launches (n <= 8, their
 * workspaces and bias gradient pointers as host arrays) into db_ih / db_hh in ONE launch, in the
 * same fixed row order (bitwise the per-launch reduce). */
#define DL4SS_RNN_DEFER_BIAS 0x400
/* precision flag of dl4ss_birnn_fwd / _fwd_ex / _fwd_mean / dl4ss_birnn_bwd / _bwd_ex: Keras 1's LSTM cell
 * (Bidirectional(LSTM(...)) of Cocktail/software/DL4SS_Keras/nnet.py:51-68 with Keras 1's default
 * inner_activation='hard_sigmoid').  With z = G + W_hh h + b_hh exactly as the logistic cell forms it,
 *   i, f, o = hs(z),  hs(z) = min(max(fma(0.2f, z, 0.5f), 0), 1)     (Theano's hard_sigmoid)
 *   g = tanh(z_g),  c = f c + i g,  h = o tanh(c)                      (unchanged)
 * and act holds the clipped gate values in the logistic cell's layout.  The BPTT takes the gate derivative
 * from the saved activation s as the logistic form takes s (1 - s): hs'(s) = 0.2f where 0 < s < 1, else 0;
 *   dG_i = dc g hs'(i),  dG_f = dc c_prev hs'(f),  dG_o = dh tanh(c) hs'(o);  dG_g, dc, dc_next unchanged.
 * A flag, not a third cell id: the gate count, the layouts, the plan (dl4ss_birnn_plan_info) and the
 * workspace size are DL4SS_CELL_LSTM's.  Accepted only with cell == DL4SS_CELL_LSTM and base precision 0 (the
 * generic fp32 kernels, any H <= 640); every other combination returns hipErrorInvalidValue before any
 * launch or device call: DL4SS_CELL_GRU, precision 1, out_bf16 / hprev_bf16 / h_mean, dG_bf16 / dGh_bf16 and
 * DL4SS_RNN_DOUT_SLABS.  (Keras's GRU is not this flag on DL4SS_CELL_GRU: besides hard_sigmoid it applies the
 * reset gate to h before the recurrent product, n = tanh(W x + U (r h)), where torch's -- this library's --
 * applies it after, n = tanh(W x + r (U h + b)): a different cell, not built.) */
#define DL4SS_RNN_HARD_GATES 0x800
/* precision field of dl4ss_birnn_bwd_ex (bits 12-13: S - 1): dOut is not one (B, T, 2H) array but the S
 * (2..4) fp32 split-K slabs dl4ss_gemm_bf16_gl leaves with DL4SS_EPI_SPLIT_SLABS, slab z at dOut + z B T 2H;
 * the BPTT sums them per element in slab order from zero (((0 + s0) + s1) + ...), bitwise the combine
 * launch it replaces.  Packed bf16 BPTT at batch chunks of 4 only (hipErrorInvalidValue otherwise). */
#define DL4SS_RNN_DOUT_SLABS(S) ((((S) - 1) & 3) << 12)
#define DL4SS_RNN_DOUT_SLABS_MASK 0x3000
int dl4ss_birnn_bias_reduce(int cell, int B, int H, int n, void* const* workspaces, float* const* db_ih,
                            float* const* db_hh, void* stream);
/* dl4ss_birnn_bias_reduce with db = beta db + sums: beta 0 writes db_ih / db_hh without reading them
 * (the training step then needs no zeroed gradient buffer; beta 1 is bitwise the += form). */
int dl4ss_birnn_bias_reduce_ex(int cell, int B, int H, int n, void* const* workspaces, float* const* db_ih,
                               float* const* db_hh, float beta, void* stream);
long long dl4ss_birnn_workspace_bytes(int cell, int B, int H);
/* The persistent recurrence's plan under a co-residency budget: every workgroup of a launch
 * (2 directions x nchunk batch chunks x NG units groups) must be resident at once, so the
 * batch chunk BC is the smallest in {1, 2, 4, 8} with 2 * nchunk * NG <= max_wg (max_wg <= 0:
 * the current device's CUs minus 1/16, 240 on a full MI355X; dl4ss_debug_set_rnn_max_wg overrides).
 * info[5] = {BC, NG, J, nchunk, grid}.  Host-only when max_wg > 0.  0, or
 * hipErrorInvalidValue when no plan fits.  Every launch re-checks the grid against the CU
 * count x the kernel's occupancy and fails with hipErrorCooperativeLaunchTooLarge (720)
 * instead of spinning to the hand-off timeout. */
int dl4ss_birnn_plan_info(int cell, int B, int H, int precision, int max_wg, int* info);
/* Test hook: polls before a recurrence hand-off times out (0 = default, ~1 s of polling). */
void dl4ss_debug_set_spin_limit(unsigned limit);
/* Test hook: 1 = the packed (bf16) recurrence kernels write every hand-off granule through
 * (`sc1`), as for a group whose workgroups span XCDs; 0 = by the placement found at launch. */
void dl4ss_debug_set_place_force(int force);
/* Test hook: > 0 replaces the device's co-residency budget (workgroups per persistent launch) in
 * every later recurrence plan -- e.g. 120 gives the B = 32, H = 300 nets batch chunks of 8, the
 * plan of B >= 33 on a full MI355X; 0 restores the default. */
void dl4ss_debug_set_rnn_max_wg(int max_wg);
/* One layer, both directions: G (B,T,2,NG*H) = X W_ih^T + b_ih (NG = 4 LSTM / 3 GRU),
 * W_hh (2, NG*H, H), b_hh (2, NG*H) -> out (B,T,2H) [fwd | reverse], hprev (B,T,2H)
 * (h_{t-1} per step), act (B,T,2,4H) gate activations, cs (B,T,2,H) LSTM cells.  act is
 * gate-major (B,T,2,4H) except where both packed bf16 kernels run the plan at batch chunks >= 4
 * (every C2 / C4 step at B = 32): there it is cell-major (B,T,2,H,4), one 16-B record per cell,
 * written by the forward and read by dl4ss_birnn_bwd[_ex] of the same precision and shape.
 * precision 0: exact fp32 recurrent matvec (VALU); 1: bf16 operands on MFMA with fp32
 * accumulate (cell state, gates and all outputs stay fp32).  A precision-0 plan that does not
 * fit the co-residency budget at B (H = 600: 50 workgroups per group, B <= 16 on a full part)
 * runs as consecutive near-equal sub-batch launches on the same workspace (rows never interact;
 * dl4ss_birnn_workspace_bytes sizes the workspace for the sub-batch plan).
 * *status != 0 after the call means a hand-off timed out (results invalid).
 * Replaces the cuDNN recurrence of nn.LSTM / nn.GRU(batch_first, bidirectional)
 * at TDAA_beta/main_run_sstune_EvalVer.py:282-293, Torch_multi/main_run.py:263-273. */
int dl4ss_birnn_fwd(int cell, int precision, int B, int T, int H, const float* G, const float* W_hh,
                    const float* b_hh, float* out, float* hprev, float* act, float* cs, void* workspace,
                    long long ws_bytes, int* status, void* stream);
/* dl4ss_birnn_fwd with bf16 extras (precision 1, packed-hand-off kernel only):
 * out_bf16 (B*T rows of pad8(2H): [fwd | reverse] adjacent) receives bf16(h), the next
 * layer's / the Linear's GEMM operand; hprev_bf16 (B*T rows of 2 pad8(H): each direction's
 * block 16-B aligned) receives bf16(h_{t-1}), the W_hh weight-gradient operand
 * (pad8(n) = n rounded up to a multiple of 8; pads are not written).  hprev may be NULL
 * for LSTM (only the GRU BPTT reads the fp32 h_{t-1}). */
int dl4ss_birnn_fwd_ex(int cell, int precision, int B, int T, int H, const float* G, const float* W_hh,
                       const float* b_hh, float* out, float* hprev, float* act, float* cs, void* out_bf16,
                       void* hprev_bf16, void* workspace, long long ws_bytes, int* status, void* stream);
/* dl4ss_birnn_fwd_ex with, in the packed kernel (precision 1), the fp32 output optional (out NULL when
 * out_bf16 is given) and h_mean (B, 2H) = the mean over t of the output, summed in step order by each
 * unit's cell lane (NULL: none) -- as dl4ss_birnn_fwd_xw_ex, for the unfused projection. */
int dl4ss_birnn_fwd_mean(int cell, int precision, int B, int T, int H, const float* G, const float* W_hh,
                         const float* b_hh, float* out, float* hprev, float* act, float* cs, void* out_bf16,
                         void* hprev_bf16, float* h_mean, void* workspace, long long ws_bytes, int* status, void* stream);
/* dl4ss_birnn_fwd_ex with the input projection fused into the recurrence (bf16 packed kernel):
 * no G buffer and no separate GEMM -- every workgroup forms x_t W_ih^T + b_ih of its own gate rows
 * with MFMAs while the previous step's hand-off travels.  x_bf16 (B*T, ldx) bf16 layer input rows
 * (read in 16-B chunks: the row padding up to the next multiple of 8 must be finite, e.g. zero), W_ih_bf16 (2*NGATE*H, ldw) bf16, b_ih (2, NGATE*H); ldx, ldw multiples of 8,
 * x_bf16 and W_ih_bf16 16-B aligned.  Bitwise equal to gemm_gl (G = x W_ih^T + b_ih) followed by
 * dl4ss_birnn_fwd_ex.  Replaces the same reference lines as dl4ss_birnn_fwd (the cuDNN LSTM / GRU of
 * TDAA_beta/main_run_sstune_EvalVer.py:282-293, whose input projection is part of that call).
 * ws_zeroed: the caller already zeroed the hand-off area. */
int dl4ss_birnn_fwd_xw(int cell, int B, int T, int H, const void* x_bf16, int Kin, long long ldx,
                       const void* W_ih_bf16, long long ldw, const float* b_ih, const float* W_hh,
                       const float* b_hh, float* out, float* hprev, float* act, float* cs, void* out_bf16,
                       void* hprev_bf16, void* workspace, long long ws_bytes, int* status, void* stream,
                       int ws_zeroed);
/* dl4ss_birnn_fwd_xw with the fp32 layer output optional (out may be NULL when out_bf16 is not)
 * and h_mean (B, 2H) (NULL: none) = the mean over t of the layer output, each (b, direction, unit)
 * summed in step order by the unit's own cell lane -- the time mean of the last layer that ADDJUST
 * (EvalVer.py:363-377) reads, without a pass over the output. */
int dl4ss_birnn_fwd_xw_ex(int cell, int B, int T, int H, const void* x_bf16, int Kin, long long ldx,
                          const void* W_ih_bf16, long long ldw, const float* b_ih, const float* W_hh, const float* b_hh,
                          float* out, float* hprev, float* act, float* cs, void* out_bf16, void* hprev_bf16,
                          float* h_mean, void* workspace, long long ws_bytes, int* status, void* stream, int ws_zeroed);
/* 1 when dl4ss_birnn_fwd_xw applies to (cell, B, T, H, Kin) (the packed bf16 plan exists, Kin <= 640);
 * host-only. */
int dl4ss_birnn_fwd_xw_supported(int cell, int B, int T, int H, int Kin);
/* BPTT of one layer: dOut (B,T,2H) (+ dOut_bcast (B,2H) at every t, may be NULL) ->
 * dG (B,T,2,NG*H) grad of the input projection (pre-activation) and, for GRU, dGh
 * grad of W_hh h + b_hh (for LSTM they coincide; dGh may be NULL).  The mask nets' entry point:
 * H <= 320 (a wider layer is refused here; dl4ss_birnn_bwd_ex runs it). */
int dl4ss_birnn_bwd(int cell, int precision, int B, int T, int H, const float* dOut, const float* dOut_bcast,
                    const float* W_hh, const float* act, const float* cs, const float* hprev, float* dG, float* dGh, void* workspace,
                    long long ws_bytes, int* status, void* stream);

/* dl4ss_birnn_bwd with bf16 extras (precision 1, packed-hand-off kernel only): dG_bf16 /
 * dGh_bf16 (B,T,2,NG*H) receive bf16 copies (the weight-gradient / dX GEMM operands),
 * dG / dGh may then be NULL, and db_ih / db_hh (2, NG*H) are ACCUMULATED with the sums
 * over (b,t) of dG / dGh (the bias gradients: each cell's sum over t in step order goes to a per-row
 * partial in the workspace, a fixed-order reduce adds the rows -- no atomics, bitwise repeatable).
 * Large hidden sizes (320 < H <= 640; H > 640 is refused before any device call): the BPTT of the
 * H = 600 speaker classifier, loss.backward() through nn.LSTM(129, 600, 3, bidirectional) at
 * Torch_multi/test_multi_labels_speech.py:444 (:240-246).  Generic kernel only (precision 0 or 1, both
 * cells, gate-major act as the large-H forward writes it): no bf16 copies, no fused bias sums, no dOut
 * slabs, fp32 dG (and dGh for GRU) required.  Wherever the generic kernel runs (every H > 320 plan,
 * precision 0, bf16 plans without the packed form) dOut may be NULL (read as zero) when dOut_bcast is
 * given: the classifier's top layer, whose only gradient is d(mean_t h).  A precision-0 plan that does not fit
 * the co-residency budget at B runs as the forward's sub-batch launches (see dl4ss_birnn_fwd). */
int dl4ss_birnn_bwd_ex(int cell, int precision, int B, int T, int H, const float* dOut, const float* dOut_bcast,
                       const float* W_hh, const float* act, const float* cs, const float* hprev, float* dG,
                       float* dGh, void* dG_bf16, void* dGh_bf16, float* db_ih, float* db_hh, void* workspace,
                       long long ws_bytes, int* status, void* stream);

/* ---- speaker-query mask attention + loss (fused forward/backward) -------- */
/* Blocks per utterance used by the partial-sum buffers. */
int dl4ss_attn_nblk(int T, int F);
/* pass 0 (COST): costs (+ optional mask / pred outputs); pass 1 (GRAD): also
 * dPre (B,T*F,E) = dL/d(h W_lin^T + b) (may alias V: in-place) and dq partials.
 * V (B,T*F,E) = tanh Linear output; q (B,K,QW), QW = E (magnitude) or 2E (cRM).
 * X: magnitude (b*x_bstride + row) or complex [re,im] pairs; Y target k of b at
 * b*y_bstride + k*y_kstride (+ row).  perm (B,K) target per channel (NULL = label
 * order).  s1/s2 scale the MSE and sum-to-one terms.  part_loss (B,nblk,K*K+1),
 * part_dq (B,nblk,K,QW).
 * Replaces EvalVer.py:615-666 (expand + baddbmm + sigmoid + MSE + sum loss) and
 * main_run_sstune_cRM_EvalVer.py:259-271,688,720-743 (cRM branch). */
int dl4ss_mask_attn_loss(int pass, int crm, int B, int K, int T, int F, int E, const float* V, const float* q,
                         const float* X, long long x_bstride, const float* Y, long long y_bstride,
                         long long y_kstride, const int* perm, float s1, float s2, float* dPre, float* part_loss,
                         float* part_dq, float* mask_out, float* pred_out, void* stream);
/* dl4ss_mask_attn_loss with a bf16 GRAD output: dPre_bf16 row (b*T + t) holds the F*E
 * values of frame t at stride dpre_bf16_ld (even, >= F*E: 16-B rows for the Linear's
 * backward GEMMs); dPre may then be NULL.  A non-NULL dPre_bf16 on the magnitude path (also
 * given to the COST pass, which does not write it) selects the quad-per-row kernel for the fp32
 * V as well -- logits summed as quad partials, as the bf16-V kernel does; NULL keeps the
 * row-per-lane kernel of the fp32 parity step. */
int dl4ss_mask_attn_loss_ex(int pass, int crm, int B, int K, int T, int F, int E, const float* V, const float* q,
                            const float* X, long long x_bstride, const float* Y, long long y_bstride,
                            long long y_kstride, const int* perm, float s1, float s2, float* dPre, void* dPre_bf16,
                            long long dpre_bf16_ld, float* part_loss, float* part_dq, float* mask_out,
                            float* pred_out, void* stream);
/* dl4ss_mask_attn_loss_ex with V in bf16 (V_bf16: (B, T*F, E) raw 16-bit words, 4-B aligned):
 * the bf16 path's Linear writes V = tanh(h W^T + b) directly in bf16 (gemm EPI_TANH_BF16),
 * halving the bytes of the Linear's output and of both attention passes' V reads. */
int dl4ss_mask_attn_loss_bf16v(int pass, int crm, int B, int K, int T, int F, int E, const void* V_bf16, const float* q,
                               const float* X, long long x_bstride, const float* Y, long long y_bstride,
                               long long y_kstride, const int* perm, float s1, float s2, float* dPre, void* dPre_bf16,
                               long long dpre_bf16_ld, float* part_loss, float* part_dq, float* mask_out,
                               float* pred_out, void* stream);
/* The magnitude path's GRAD pass (pass 1, crm 0 of dl4ss_mask_attn_loss_ex) with a second gradient at the
 * prediction pred = mask |X|: dpred_extra (B, K, T*F) fp32 in pred_out's layout, e.g. the Discriminator's
 * input gradient on the predicted maps (the adversarial step: dis.py:642-646, loss_multi_speech + the
 * "fake looks real" term).  dm = (2 s1 (m x - y) + dpred_extra) x + 2 s2 ds; the loss partials are those of
 * the call without it, bit for bit.  K = 1..3, E = 50.  The kernel form follows dPre_bf16 as in _ex. */
int dl4ss_mask_attn_loss_adv(int B, int K, int T, int F, int E, const float* V, const float* q, const float* X,
                             long long x_bstride, const float* Y, long long y_bstride, long long y_kstride,
                             const int* perm, float s1, float s2, const float* dpred_extra, float* dPre,
                             void* dPre_bf16, long long dpre_bf16_ld, float* part_loss, float* part_dq,
                             float* mask_out, float* pred_out, void* stream);
/* dl4ss_mask_attn_loss_adv with V in bf16 (as dl4ss_mask_attn_loss_bf16v). */
int dl4ss_mask_attn_loss_adv_bf16v(int B, int K, int T, int F, int E, const void* V_bf16, const float* q,
                                   const float* X, long long x_bstride, const float* Y, long long y_bstride,
                                   long long y_kstride, const int* perm, float s1, float s2,
                                   const float* dpred_extra, float* dPre, void* dPre_bf16, long long dpre_bf16_ld,
                                   float* part_loss, float* part_dq, float* mask_out, float* pred_out,
                                   void* stream);
/* PIT: per utterance the lowest-index permutation minimising the summed costs. */
int dl4ss_pit_select(const float* part_loss, int B, int K, int nblk, int* perm, void* stream);
/* loss_out[3] = {total, MSE term, weighted sum-to-one term}; dq = sum of partials. */
int dl4ss_loss_finalize(const float* part_loss, int B, int K, int nblk, const int* perm, float s1, float s2,
                        float* loss_out, const float* part_dq, int qw, float* dq, void* stream);

/* ---- speaker queries, reductions, optimizer ------------------------------ */
/* q[b,k] = Emb[idx[b,k]] (+ W_adj [mean_t h[b]; Emb[idx[b,k]]]); h (B,T,D).
 * SPEECH_EMBEDDING + ADDJUST: EvalVer.py:348-377,606-608. w_adj may be NULL; an idx of -1 (no speaker) gives a zero
 * query, with w_adj too (the W_adj . mean part belongs to no speaker), and its dq reaches no gradient of
 * dl4ss_query_bwd[_ex] (d_emb, d_wadj or dh_bcast).
 * mean_out (B,D) receives mean_t h; with h NULL it is instead READ as that mean, formed by the
 * recurrence (dl4ss_birnn_fwd_xw_ex h_mean). */
int dl4ss_query_fwd(const float* h, int B, int T, int D, const int* idx, const float* emb, const float* w_adj, int K,
                    int W, float* q, float* mean_out, void* stream);
/* d_emb (+=, scatter), d_wadj (+=), dh_bcast (B,D) = W_m^T sum_k dq / T. */
int dl4ss_query_bwd(const float* dq, int B, int T, int D, const int* idx, const float* emb, const float* w_adj,
                    const float* mean, int K, int W, float* d_emb, float* d_wadj, float* dh_bcast, void* stream);
/* dl4ss_query_bwd with d_emb / d_wadj = beta (old) + this step's: beta 0 writes them without reading --
 * every d_wadj element, the embedding rows the batch's speakers own, and zeros in the other rows of
 * the n_labels-row d_emb (the step's gradient buffer then needs no zeroing pass); beta 1 is bitwise
 * dl4ss_query_bwd (n_labels unused). */
int dl4ss_query_bwd_ex(const float* dq, int B, int T, int D, const int* idx, const float* emb, const float* w_adj,
                       const float* mean, int K, int W, float* d_emb, float* d_wadj, float* dh_bcast, int n_labels,
                       float beta, void* stream);
/* out[n] += sum_m A[m*lda + n] (bias gradients). */
int dl4ss_colsum(const float* A, long long lda, int M, int N, float* out, void* stream);
/* torch.optim.Adam step on flat fp32 buffers (EvalVer.py:538-544). */
int dl4ss_adam(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
               float eps, int step, void* stream);
/* dl4ss_adam that refuses a step computed from a timed-out recurrence: when status[0] != 0
 * (a BiRNN hand-off of this step timed out) no parameter or moment changes and loss[0] (if not
 * NULL) is set to NaN, so the step's loss read by the caller reports it.  status is ONE int,
 * only read. */
int dl4ss_adam_guarded(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                       float beta2, float eps, int step, int* status, float* loss, void* stream);
/* dl4ss_adam_guarded that also refuses when *dp_flag != 0: the data-parallel form, where
 * dp_flag is the slot behind the flat gradient that dl4ss_status_flag filled from each rank's
 * status and the gradient all-reduce combined, so every rank refuses the same steps.  Here
 * status points at 2 ints: {hand-off word, refused-update count}; the count is incremented on
 * every refusal (the host rolls its Adam step count back by it). */
int dl4ss_adam_guarded_dp(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                          float beta2, float eps, int step, int* status, const float* dp_flag, float* loss,
                          void* stream);
/* dl4ss_adam_guarded_dp on g * gscale: the data-parallel step takes the gradient all-reduced with
 * SUM and applies the 1 / world_size of the mean here (no separate pass over the buffer; gscale =
 * 1 is bitwise the unscaled step).  Replaces optimizer.step() at EvalVer.py:673-675 under DP. */
int dl4ss_adam_guarded_dp_scaled(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                                 float beta2, float eps, int step, int* status, const float* dp_flag, float gscale,
                                 float* loss, void* stream);
/* dl4ss_adam_guarded_dp_scaled that also writes bf16 (round-to-nearest-even) shadow copies of the
 * updated parameters: segment s < nseg (<= 8) maps the flat range [seg_off[s], + rows*cols) row-major
 * onto seg_y[s] (row stride seg_ldy[s] >= cols; columns >= cols untouched).  The bf16 step's weight
 * operands (W_ih of every layer, the Linear) then need no conversion launch before the next forward:
 * bitwise dl4ss_f32_to_bf16_2d_multi of the new parameters; a refused update leaves both untouched. */
int dl4ss_adam_guarded_dp_scaled_bf16(float* p, const float* g, float* m, float* v, long long n, float lr,
                                      float beta1, float beta2, float eps, int step, int* status, const float* dp_flag,
                                      float gscale, float* loss, int nseg, const long long* seg_off,
                                      const int* seg_rows, const int* seg_cols, void* const* seg_y,
                                      const long long* seg_ldy, void* stream);
/* ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_ on the global-batch mean gradient) ----
 * The number of fp64 partials dl4ss_grad_sumsq writes for n elements: 1 .. 1024, a function of n alone
 * (not of the device), so the same gradient gives the same bits on a full part and on a partition.  Host only. */
long long dl4ss_grad_sumsq_parts(long long n);
/* part[j] = the fp64 sum of g[i]^2 over the j-th fixed contiguous range of g (each element widened to fp64):
 * a fixed order, no atomics, bitwise reproducible.  g must be 16-B aligned. */
int dl4ss_grad_sumsq(const float* g, long long n, double* part, void* stream);
/* dl4ss_adam_guarded_dp_scaled_bf16 on the clipped gradient.  From S = sum part[0 .. n_part), in fp64 on the
 * device:  nrm = gscale sqrt(S);  c = min(1, max_norm / (nrm + 1e-6));  f = (float)(gscale c), used where
 * gscale is (c == 1: bitwise the unclipped update; max_norm = +inf measures and guards only).  gnorm (2
 * floats, may be NULL) receives {nrm, c}.  S not finite (an Inf or NaN in g): the update is refused as a
 * timed-out one is (nothing changes, loss[0] = NaN, status[1] += 1) and nonfinite[0] += 1; a hand-off time-out
 * (status[0], dp_flag) takes precedence and leaves nonfinite and gnorm alone.  part NULL: the unclipped entry. */
int dl4ss_adam_clipped(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                       float eps, int step, int* status, const float* dp_flag, float gscale, float* loss, int nseg,
                       const long long* seg_off, const int* seg_rows, const int* seg_cols, void* const* seg_y,
                       const long long* seg_ldy, const double* part, int n_part, float max_norm, float* gnorm,
                       int* nonfinite, void* stream);
/* flag[0] = status[0] != 0 ? 1 : 0 (one float, written in front of the flat gradient before its all-reduce). */
int dl4ss_status_flag(const int* status, float* flag, void* stream);

/* ---- kernels behind the reference-API nn.Modules (dl4ss_amd/compat/myNet.py) ---- */
/* dpre = dv * (1 - v^2): backward of MIX_SPEECH's tanh(Linear) (EvalVer.py:298-299). */
int dl4ss_tanh_bwd(const float* v, const float* dv, float* dpre, long long n, void* stream);
/* Row blocks of the ATTENTION 'dot' backward (size of part_dq: Bq * nblk * E). */
int dl4ss_attn_dot_nblk(int R);
/* ATTENTION 'dot': mask (Bq,R) = act(V (Bq,R,E) . q (Bq, row stride q_stride)); act 0 =
 * sigmoid (EvalVer.py:216-226), 1 = 10 tanh, the cRM branch per query half (cRM:259-271). */
int dl4ss_attn_dot_fwd(const float* V, const float* q, int q_stride, int Bq, int R, int E, int act, float* mask,
                       void* stream);
/* Its backward: dV += dE q (may be NULL; accumulates, so both cRM halves add) and
 * dq (Bq,E) = sum_r dE V (deterministic partial sums, part_dq: Bq*nblk*E). */
int dl4ss_attn_dot_bwd(const float* V, const float* q, int q_stride, const float* mask, const float* dmask, int Bq,
                       int R, int E, int act, float* dV, float* part_dq, float* dq, void* stream);
/* top_k_mask (EvalVer.py:390-405, main_run.py:340-355): mask (B,N) of the first
 * min(top_k, #{p > alpha}) entries in descending order (ties: lower index first);
 * idx (B,top_k) the selected ids ascending (-1 padded), count (B); idx/count may be NULL. */
int dl4ss_top_k_mask(const float* prob, int B, int N, float alpha, int top_k, float* mask, int* idx, int* count,
                     void* stream);
/* dl4ss_attn_dot_fwd with an output row stride: mask[b * mask_stride + r] (K queries of one
 * V (B,R,E) write a (B,K,R) mask without expanding V, the 414 MB copy of EvalVer.py:615-617). */
int dl4ss_attn_dot_fwd_ex(const float* V, const float* q, int q_stride, int Bq, int R, int E, int act, float* mask,
                          long long mask_stride, void* stream);

/* ---- ATTENTION 'align' (additive attention) ---- */
/* mask = sigmoid(w3 . tanh(W1 V + W2 q)): Cocktail/software/DL4SS_Keras/extend_layers.py:50-64
 * (built by default, nnet.py:88) and the 'align' branch of the Torch ATTENTION classes
 * (TDAA_beta/main_run_sstune_EvalVer.py:228-239).  W1 = Linear_1.weight (E,E), W2 =
 * Linear_2.weight (E,E), w3 = Linear_3.weight (1,E), no biases; E = 50 only. */
/* Blocks per utterance of R rows (part_loss is (B, nblk, K*K+1) as for dl4ss_mask_attn_loss). */
int dl4ss_attn_align_nblk(int R);
/* Floats of the backward's partial-sum workspace `part` for B utterances of nblk blocks and K
 * queries each (the module-level backward: B = Bq, K = 1); -1 for an unsupported K. */
long long dl4ss_attn_align_part_floats(int B, int K, int nblk);
/* Module level, forward: mask[b * mask_stride + r], V (Bq,R,E), the query of b at q + b * q_stride
 * (K queries of one V write a (B,K,R) mask with mask_stride = K*R, as dl4ss_attn_dot_fwd_ex). */
int dl4ss_attn_align_fwd(const float* V, const float* q, int q_stride, const float* W1, const float* W2,
                         const float* w3, int Bq, int R, int E, float* mask, long long mask_stride, void* stream);
/* Its backward from dmask (Bq,R), s and the mask recomputed from V: dV (Bq,R,E) += dU W1 (may be
 * NULL), and dq (Bq,E), dW1, dW2, dw3 written.  Per-block partials in `part` (part_floats >=
 * dl4ss_attn_align_part_floats(Bq, 1, dl4ss_attn_align_nblk(R))), summed in fixed order: no atomics. */
int dl4ss_attn_align_bwd(const float* V, const float* q, int q_stride, const float* W1, const float* W2,
                         const float* w3, const float* dmask, int Bq, int R, int E, float* dV, float* part,
                         long long part_floats, float* dq, float* dW1, float* dW2, float* dw3, void* stream);
/* The fused step kernel, the 'align' counterpart of dl4ss_mask_attn_loss on fp32 V (magnitude path;
 * the loss of EvalVer.py:641,659-666): pass 0 COST, pass 1 GRAD, with that entry point's V / q (B,K,E)
 * / X / Y / strides / perm / s1 / s2 / mask_out / pred_out contract; part_loss (B,nblk,K*K+1), nblk =
 * dl4ss_attn_align_nblk(T*F), feeds dl4ss_pit_select and dl4ss_loss_finalize (with dq NULL) unchanged.
 * GRAD writes dPre (B,T*F,E) (may be V itself: in place) and the partials of dp, dW1, dw3 into `part`
 * (part_floats >= dl4ss_attn_align_part_floats(B, K, nblk)); dl4ss_attn_align_finalize forms the
 * gradients from them. */
int dl4ss_mask_attn_align_loss(int pass, int B, int K, int T, int F, int E, const float* V, const float* q,
                               const float* W1, const float* W2, const float* w3, const float* X,
                               long long x_bstride, const float* Y, long long y_bstride, long long y_kstride,
                               const int* perm, float s1, float s2, float* dPre, float* part_loss, float* part,
                               long long part_floats, float* mask_out, float* pred_out, void* stream);
/* dq (B,K,E), dW1 (E,E), dW2 (E,E), dw3 (E), written, from the GRAD pass's `part` (q, W2 as given
 * to it): the block partials summed in block order, dq = dp W2, dW2 = sum_{b,k} dp (x) q. */
int dl4ss_attn_align_finalize(const float* part, long long part_floats, int B, int K, int T, int F, const float* q,
                              const float* W2, float* dq, float* dW1, float* dW2, float* dw3, void* stream);

/* ---- recursive extraction / speaker classifier ---- */
/* Speaker choice of one recursion step (Torch_multi/main_run_multi_selfSS_recuReal_GRID.py:
 * 227-244 top_k_mask with sort_index, 391-404 the seen-speaker filter), per row b:
 * prob = sigmoid(logits) (GRID.py:197; may be NULL), sort_index (B,top_k) ids by descending
 * prob (ties: lower id; -1 beyond N; may be NULL), chosen (B) = first id of sort_index not in
 * prev (n_prev,B) (the ids chosen at earlier steps, -1 = none) if any prob > alpha, else -1
 * (may be NULL).  top_k <= 64, N <= 8192. */
int dl4ss_classifier_select(const float* logits, int B, int N, float alpha, int top_k, const int* prev, int n_prev,
                            float* prob, int* sort_index, int* chosen, void* stream);
/* pred = mask * x and resid = (1 - mask) * x, n elements (GRID.py:433-434 predict_multi_map,
 * GRID.py:444 the residual spectrogram); pred or resid may be NULL. */
int dl4ss_mask_split(const float* mask, const float* x, long long n, float* pred, float* resid, void* stream);
/* mean over t of h (B,T,D) -> (B,D): the classifier's torch.mean(x, 1) (GRID.py:196,
 * EvalVer.py:323) and ADDJUST's time mean (EvalVer.py:373). */
int dl4ss_time_mean(const float* h, int B, int T, int D, float* mean_out, void* stream);
/* Classifier head forward: m (B, D) the time mean of the top BiLSTM layer (D = 2H), W (C, D), b (C)
 * -> logits z (B, C) and p = sigmoid(z): self.Linear + F.sigmoid of MIX_SPEECH_classifier
 * (Torch_multi/test_multi_labels_speech.py:259-263).  No allocation; B <= 65535. */
int dl4ss_cls_head_fwd(const float* m, const float* W, const float* b, int B, int D, int C, float* z, float* p,
                       void* stream);
/* Classifier loss and head backward of one training step (test_multi_labels_speech.py:397,437,444):
 * nn.MultiLabelSoftMarginLoss applied, as the reference does, to the sigmoid output p (not the logits)
 * against the multi-hot y (B, C), and its gradient through sigmoid, Linear and the time mean over T:
 *   loss (1) = -1/(B C) sum [ y log sigmoid(p) + (1 - y) log sigmoid(-p) ]
 *   dz (B, C) = (sigmoid(p) - y) / (B C) * p (1 - p),  dW (C, D) = dz^T m,  db (C) = sum_b dz,
 *   dOut_bcast (B, D) = dz W / T  -- the constant-over-t dOut term of the top layer's BPTT
 *   (dl4ss_birnn_bwd_ex with dOut NULL).
 * All outputs are written; fixed-order sums, no atomics (repeatable bit for bit); no allocation. */
int dl4ss_cls_head_loss_bwd(const float* p, const float* y, const float* m, const float* W, int B, int D, int C,
                            int T, float* loss, float* dz, float* dW, float* db, float* dOut_bcast, void* stream);

/* ---- Discriminator (TDAA_beta/main_run_sstune_dis.py:318-336,615-647; the same class in
 * main_run_sstune_EvalVer.py:328-346): Conv2d(1, 64, 3x3, stride 2) + two Conv2d(64, 64, 3x3, stride 2),
 * ReLU after each, Linear(64 H3 W3, 1) + sigmoid, MSE against 1 / 0, and their autograd.
 * Activations are channels-last (N, H, W, 64), fp32 (prec 0) or bf16 (prec 1); parameters and their
 * gradients are fp32 in the reference's layouts (conv weight (64, Cin, 3, 3), final.weight flattened
 * (c, h, w)).  Hout = (Hin - 3) / 2 + 1 per layer and axis.  No float atomics: two calls on the same
 * inputs agree bit for bit.  Sizes are checked before any device call. */
/* hw = {H1, W1, H2, W2, H3, W3} of a (T, F) map; returns the feature count 64 H3 W3, or -1 when the map is
 * smaller than 15 x 15.  Host only (hw may be NULL). */
int dl4ss_disc_dims(int T, int F, int hw[6]);
/* Bytes of the workspace the *_bwd calls of N maps of (T, F) share (split-K partials of the largest
 * layer), or -1 for an unsupported size.  Host only. */
long long dl4ss_disc_ws_bytes(int N, int T, int F);
/* x (N, T, F) fp32, w (64, 1, 3, 3), b (64) -> y1 (N, H1, W1, 64) = relu(conv + b); fp32 arithmetic, the
 * output alone is rounded in bf16. */
int dl4ss_disc_conv1_fwd(int prec, const float* x, const float* w, const float* b, int N, int T, int F, void* y1,
                         void* stream);
/* x (N, Hin, Win, 64), w (64, 64, 3, 3), b (64) -> y (N, Hout, Wout, 64) = relu(conv + b): implicit GEMM on
 * the MFMA (M = N Hout Wout, N = 64, K = 576), rows gathered from the nine taps. */
int dl4ss_disc_conv64_fwd(int prec, const void* x, const float* w, const float* b, int N, int Hin, int Win, void* y,
                          void* stream);
/* y3 (N, H3, W3, 64), wf (64 H3 W3), bf (1) -> z (N), score (N) = sigmoid(z) */
int dl4ss_disc_head_fwd(int prec, const void* y3, const float* wf, const float* bf, int N, int H3, int W3, float* z,
                        float* score, void* stream);
/* Head backward.  dscore (N) given: dz = dscore s (1 - s).  dscore NULL: the fused loss
 * loss[0] = mean_n (score_n - target)^2 (dis.py:622-624,642) and its gradient.  Writes dz (N), dwf, dbf (1)
 * and dy3 (N, H3, W3, 64) in the activation type; loss may be NULL. */
int dl4ss_disc_head_bwd(int prec, const void* y3, const float* wf, const float* score, const float* dscore,
                        float target, int N, int H3, int W3, float* loss, float* dz, float* dwf, float* dbf, void* dy3,
                        void* stream);
/* The adversarial step's loss heads (dis.py:622-624,642): score (2 N) = [D(true maps); D(predicted maps)] ->
 * loss (3) = {mean (s_true - 1)^2, mean s_fake^2, mean (s_fake - 1)^2}, dscore_dis (2 N) = the gradient of
 * the first two at every score, dscore_adv (N) = lambda times the third's at the predicted maps' scores;
 * both feed dl4ss_disc_head_bwd's dscore.  Fixed summation order. */
int dl4ss_disc_adv_heads(const float* score, int N, float lambda, float* loss, float* dscore_dis, float* dscore_adv,
                         void* stream);
/* 64 -> 64 layer backward from dy and the saved post-ReLU y (gate y > 0 applied on load): dw (64, 64, 3, 3),
 * db (64) and, when dx is not NULL, dx (N, Hin, Win, 64) with every element written (exact zeros where no
 * window reaches).  ws / ws_bytes: dl4ss_disc_ws_bytes of the network this layer belongs to. */
int dl4ss_disc_conv64_bwd(int prec, const void* x, const void* y, const void* dy, const float* w, int N, int Hin,
                          int Win, void* dx, float* dw, float* db, void* ws, long long ws_bytes, void* stream);
/* conv1 backward: dw (64, 1, 3, 3), db (64) and, when dx is not NULL, the input-map gradient dx (N, T, F) fp32. */
int dl4ss_disc_conv1_bwd(int prec, const float* x, const void* y1, const void* dy1, const float* w, int N, int T,
                         int F, float* dx, float* dw, float* db, void* ws, long long ws_bytes, void* stream);

/* ---- voiceprint encoder and speaker memory (Cocktail/software/DL4SS_Keras/nnet.py:64-92,
 *      extend_layers.py:105-228): a speaker enrolled from clean speech.  fp32; no atomics, every sum in a
 *      fixed order (repeatable bit for bit); sizes are checked before any device call. ---- */
/* Frame mask and compaction.  x (n, T, F) -> xc (n, T, F): utterance b's valid frames in their own order as
 * rows [0, len[b]), zero rows behind; len (n) int32; idx (n, T) int32, idx[b, j] = the j-th valid frame, -1
 * for j >= len[b].  rule 0: a frame is valid when any bin != 0 (Masking(0.), nnet.py:46); rule 1: when any
 * bin > thr (MaskingGt, nnet.py:44; the caller passes log features, no logarithm is taken here).  len_in (n,
 * NULL: none) overrides the rule with the prefix [0, len_in[b]) (clamped to [0, T]).  T <= 2048; xc != x. */
int dl4ss_vp_compact(const float* x, int n, int T, int F, int rule, float thr, const int* len_in, float* xc,
                     int* len, int* idx, void* stream);
/* Row shift of the columns [c0, c1) of src (n, T, ld) into dst (same shape, dst != src) by d = T - len[b]:
 * dir +1: dst row t = src row t - d, rows < d zero (compact frame -> right-aligned, the frame in which the
 * full-length recurrence starts an utterance's reverse pass at its own last frame); dir -1: dst row t = src
 * row t + d, rows >= len[b] zero (back).  The other columns of dst: other 0 untouched, 1 = src on rows < len[b]
 * and zero beyond, 2 = src -- one launch assembles the next layer's input, or moves one direction of G / dG. */
int dl4ss_vp_shift(const float* src, float* dst, int n, int T, int ld, int c0, int c1, const int* len, int dir,
                   int other, void* stream);
/* Masked mean (MeanPool, extend_layers.py:105-125) of a layer output out (n, T, 2H) in the recurrence's frame:
 * vec (n, 2H) = sum / (len + 2.22e-16) over the forward half's rows [0, len) and the reverse half's rows
 * [T - len, T), in ascending t; len 0 gives zeros. */
int dl4ss_vp_mean_fwd(const float* out, int n, int T, int H, const int* len, float* vec, void* stream);
/* Its backward: every element of dOut (n, T, 2H) written, dvec / (len + 2.22e-16) on the rows the mean read
 * and zero elsewhere (the BPTT then yields a dG that is exactly zero on the padded rows). */
int dl4ss_vp_mean_bwd(const float* dvec, int n, int T, int H, const int* len, float* dOut, void* stream);
/* Column sums in a fixed order for any row count (the encoder's bias gradient colsum(dG); dl4ss_colsum adds
 * its row blocks atomically): out (C) = sum over the M rows of the contiguous A (M, C).  Blocks of 64 rows are
 * summed in ascending row into part (dl4ss_vp_colsum_parts(M) * C floats), then the parts in ascending block;
 * the same input gives the same bits.  Every element of out is written.  1 <= M <= 65535 * 64 (the parts query
 * returns -1 outside). */
long long dl4ss_vp_colsum_parts(long long M);
int dl4ss_vp_colsum(const float* A, long long M, int C, float* part, float* out, void* stream);
/* Speaker memory forward (extend_layers.py:149-179).  v (n, E) voiceprints, ids (n) int32, mem (M, E), read
 * only:  u_i = v_i / |w(v_i)|, w(a) = a with 2.22e-16 where a == 0;  A = mem, A[ids[i]] += u_i in ascending i
 * (duplicate ids accumulate, as inc_subtensor);  q_i = A[ids[i]] / |w(A[ids[i]])|.  An id outside [0, M) (-1:
 * no speaker) gives a zero query and adds nothing.  u (n, E) and q (n, E) are written; only the rows the
 * batch touches are formed.  n <= 1024, E <= 128; one workgroup. */
int dl4ss_spk_memory_fwd(const float* v, const int* ids, const float* mem, int n, int E, int M, float* u, float* q,
                         void* stream);
/* Its backward: dv (n, E) from dq (n, E), with v, ids, mem as given to the forward and the u it wrote.  The
 * switch passes no gradient to its constant branch; mem gets none (trainable=False). */
int dl4ss_spk_memory_bwd(const float* dq, const float* v, const float* u, const int* ids, const float* mem, int n,
                         int E, int M, float* dv, void* stream);
/* update_memory (extend_layers.py:220-228): mem[ids[i]] = q_i (duplicates carry identical rows, ids outside
 * [0, M) are skipped).  status (NULL: none): the recurrence status word; status[0] != 0 (the guarded Adam
 * refused this step) leaves mem untouched. */
int dl4ss_spk_memory_store(const float* q, const int* ids, int n, int E, int M, float* mem, const int* status,
                           void* stream);

/* ---- BSS-eval (replaces the un-vendored separation.bss_eval_sources of
 *      Torch_multi/bss_test.py:5,55 -- BSS_EVAL v3, 512-tap distortion filters) ---- */
/* R (M,P,P,L) fp64: R[m][a][b][l] = sum_n x[m][a][n] x[m][b][n+l], l < L, x (M,P,N) fp32
 * (the K references then the estimates of mixture m). */
int dl4ss_bss_corr(const float* x, int M, int P, int N, int L, double* R, void* stream);
/* From R: the Gram matrix of the delayed references G (M, K L, K L) (may be NULL), its
 * diagonal blocks Gd (M, K, L, L) (may be NULL) and D (M, K L, P-K) = <delayed refs, est>. */
int dl4ss_bss_gram(const double* R, int M, int P, int K, int L, double* G, double* Gd, double* D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DL4SS_HIP_H */
