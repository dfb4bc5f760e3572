/* dl4ss_optim.h -- C ABI of the Keras trees' optimizer in libdl4ss_hip.so (csrc/optim.hip): the third public
 * header, with the conventions of dl4ss_hip.h (int return = hipError_t, caller-owned fp32 device buffers, `stream`
 * a hipStream_t as void*, asynchronous, never allocates).
 *
 * Nadam is Keras 1's (DL4SS_Keras/nnet.py:23,113: Nadam(clipnorm=200); defaults lr 0.002, beta_1 0.9, beta_2
 * 0.999, epsilon 1e-8, schedule_decay 0.004).  With t the number of applied updates, this one included:
 *
 *   mu(i) = beta1 (1 - 0.5 0.96^(i schedule_decay)),   P(t) = mu(1) mu(2) ... mu(t)
 *   gs = g f                                   (f = gscale x the clip coefficient c, below)
 *   m' = beta1 m + (1 - beta1) gs              v' = beta2 v + (1 - beta2) gs^2
 *   p' = p - (a1 gs + a2 m') / (sqrt(v') / bc2s + eps)
 *   a1 = lr (1 - mu(t)) / (1 - P(t)),   a2 = lr mu(t+1) / (1 - P(t+1)),   bc2s = sqrt(1 - beta2^t)
 *
 * The caller passes mu = mu(t), mu_next = mu(t+1) and mu_prod = P(t) as doubles (pure functions of t); a1, a2 and
 * bc2s are formed in double here and rounded once to fp32.
 *
 * Global-norm clip: `part` is ANY array of n_part fp64 partial sums of squares, 1 <= n_part <= DL4SS_CLIP_MAX_PARTS
 * (dl4ss_grad_sumsq's of this gradient, or of several gradients side by side: every update handed the same array
 * forms the same sum S, bit for bit, and the same coefficient).  nrm = gscale sqrt(S), and
 *   clip_rule DL4SS_CLIP_TORCH:  c = min(1, max_norm / (nrm + 1e-6))     (torch.nn.utils.clip_grad_norm_)
 *   clip_rule DL4SS_CLIP_KERAS:  c = max_norm / nrm if nrm >= max_norm, else 1      (Keras's clipnorm)
 * gnorm[2] (may be NULL) receives {nrm, c}.  A sum that is not finite refuses the update: no element of p, m, v or
 * of the shadows changes, loss[0] = NaN, status[1] and nonfinite[0] go up by one, gnorm = {nrm, 0}, and with
 * nonfinite_sticky != 0 bit DL4SS_STATUS_NONFINITE_GRAD of status[0] is set and stays, so that every guarded
 * update and dl4ss_spk_memory_store behind it refuse too until the host clears the word.  part NULL: unclipped
 * (n_part, clip_rule, max_norm, gnorm, nonfinite, nonfinite_sticky are not read).
 *
 * status (2 ints: {refusal word, refused-update count}), dp_flag, gscale, loss and the shadow segments are
 * dl4ss_adam_clipped's, status may be NULL.
 */
#ifndef DL4SS_OPTIM_H
#define DL4SS_OPTIM_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DL4SS_CLIP_TORCH = 0,
  DL4SS_CLIP_KERAS = 1,
  DL4SS_CLIP_MAX_PARTS = 4096,
  DL4SS_STATUS_NONFINITE_GRAD = 4
};

/* One guarded Nadam update of the flat fp32 p from g, moments m and v (n elements each).  step >= 1;
 * 0 < mu, mu_next < 1 and 0 <= mu_prod < 1 (the product underflows to 0 in double after ~900 updates when mu stays
 * near 0.5: a valid limit, a1 = lr (1 - mu), a2 = lr mu_next). */
int dl4ss_nadam(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                float eps, int step, double mu, double mu_next, double mu_prod, int* status, const float* dp_flag,
                float gscale, float* loss, int nseg, const long long* seg_off, const int* seg_rows,
                const int* seg_cols, void* const* seg_y, const long long* seg_ldy, const double* part, int n_part,
                int clip_rule, float max_norm, float* gnorm, int* nonfinite, int nonfinite_sticky, void* stream);

/* dl4ss_adam_clipped with the clip's rule chosen and `part` relaxed as above.  clip_rule DL4SS_CLIP_TORCH with
 * dl4ss_grad_sumsq's partials of g and nonfinite_sticky 0: bitwise dl4ss_adam_clipped. */
int dl4ss_adam_clipped_ex(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                          float beta2, float eps, int step, int* status, const float* dp_flag, float gscale,
                          float* loss, int nseg, const long long* seg_off, const int* seg_rows, const int* seg_cols,
                          void* const* seg_y, const long long* seg_ldy, const double* part, int n_part,
                          int clip_rule, float max_norm, float* gnorm, int* nonfinite, int nonfinite_sticky,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DL4SS_OPTIM_H */
