/* dl4ss_eval.h -- C ABI of the target-speaker evaluation in libdl4ss_hip.so (csrc/targeteval.hip): the fourth
 * public header, with the conventions of dl4ss_hip.h (int return = hipError_t, caller-owned device buffers, `stream`
 * a hipStream_t as void*, asynchronous, never allocates, no atomics).
 *
 * The Keras trees score one extracted target speaker per mixture with BSS_EVAL.m -- BSS Eval 2.0's gain
 * decomposition (bss_decomp_gain + bss_crit) of the prediction on [noise; target] -- after building the mixture
 * from the normalised sources in a fixed order (Cocktail/software/DL4SS_Keras/predict.py:46-336).  This is a
 * different decomposition from dl4ss_bss_corr / dl4ss_bss_gram (BSS_EVAL v3, 512-tap filters): one gain per source,
 * and sources that are not to be estimated.
 */
#ifndef DL4SS_EVAL_H
#define DL4SS_EVAL_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DL4SS_BSS_GAIN_MAX_SRC = 4, /* J and Ke are 1 .. 4                                       */
  DL4SS_BSS_GAIN_CHUNK = 4096 /* samples of one utterance that one workgroup sums          */
};

/* Bytes of workspace dl4ss_bss_gain needs for M utterances of N samples (a function of M and N alone); -1 for
 * M < 0 or N < 1.  Host only. */
long long dl4ss_bss_gain_ws_bytes(int M, int N);

/* Batched BSS Eval 2.0 gain decomposition.  src (M, J, N) fp32 sources, est (M, Ke, N) fp32 estimates, index: a
 * HOST array of Ke ints, index[e] in [0, J) the source that estimate e estimates; n_eff (M) int32 on the device
 * (NULL = N): only the first n_eff[m] (clamped to [0, N]) samples of every signal of utterance m exist -- nothing
 * at or beyond is read.  With s_j, e cropped to n_eff, in fp64:
 *
 *   G = [<s_i, s_j>],  d = [<e, s_j>],  c = G^{-1} d,  P = sum_j c_j s_j,  a = <e, s_idx> / <s_idx, s_idx>
 *   s_target = a s_idx,   e_interf = P - s_target,   e_artif = e - P
 *   SDR = 10 log10(|s_target|^2 / |e_interf + e_artif|^2),  SIR = 10 log10(|s_target|^2 / |e_interf|^2),
 *   SAR = 10 log10(|s_target + e_interf|^2 / |e_artif|^2)
 *
 * crit (M, Ke, 3) fp64 = {SDR, SIR, SAR}: +inf where the denominator is 0 and the numerator is not, NaN where
 * both are.  A source of zero energy is left out of the span (c_j = 0); the rest is factored G = L D L^T in
 * ascending order, and a pivot D_j <= 1e-12 G_jj (or not a number) makes the pair singular: its three criteria are
 * NaN and it is counted.  singular[0] is WRITTEN with the number of singular (utterance, estimate) pairs of this
 * call.
 *
 * Two passes over the samples: the first forms G, d, the second accumulates sum (e - P)^2, sum (P - a s_idx)^2,
 * sum (e - a s_idx)^2 and sum P^2 from the samples themselves.  Every sum has a fixed order (a thread owns the
 * samples chunk * 4096 + lane + 256 k, a fixed shuffle tree within the wave, waves in ascending order, chunks in
 * ascending order): a repeated call returns the same bits, and utterance m's do not depend on M.
 * ws: dl4ss_bss_gain_ws_bytes(M, N) bytes, 8-B aligned.  M == 0: singular[0] = 0, nothing else. */
int dl4ss_bss_gain(const float* src, const float* est, const int* index, const int* n_eff, int M, int J, int Ke,
                   int N, void* ws, long long ws_bytes, double* crit, int* singular, void* stream);

/* The evaluation mixture in the reference's summation order (predict.py:134-158).  srcs (B, S, N) fp32: the
 * normalised, zero-padded sources (dl4ss_mix_sources_ex's out_src with gains 1; slot 0 is the target), lengths
 * (B, S) int32 their lengths (NULL = N), bgd (N) the normalised background clip (NULL = none).  From the first
 * spk_num slots (2 <= spk_num <= S <= 16), as fp32 adds in exactly this order:
 *
 *   mix    = ((s_0 + s_1) + ... + s_{spk_num-1}) [+ bgd]
 *   noise  = (s_1 + ... + s_{spk_num-1}) [+ bgd]
 *   target = s_0
 *
 * mix, noise, target (B, N) each; mix_len (B) int32 (may be NULL) = the largest length of the used sources,
 * clamped to [0, N].  No output may alias an input. */
int dl4ss_te_assemble(const float* srcs, const int* lengths, const float* bgd, int B, int S, int N, int spk_num,
                      float* mix, float* noise, float* target, int* mix_len, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DL4SS_EVAL_H */
