/* dl4ss_align.h -- C ABI of ATTENTION 'align' on the bf16 training steps in libdl4ss_hip.so (csrc/attn_align.hip):
 * the fifth public header, with the conventions of dl4ss_hip.h (int return = hipError_t, caller-owned device
 * buffers, `stream` a hipStream_t as void*, asynchronous, never allocates, no atomics).  The fp32 entry points of
 * the same attention (dl4ss_attn_align_fwd / _bwd, dl4ss_mask_attn_align_loss, dl4ss_attn_align_finalize and the
 * two size queries) stay in dl4ss_hip.h.
 */
#ifndef DL4SS_ALIGN_H
#define DL4SS_ALIGN_H

#ifdef __cplusplus
extern "C" {
#endif

/* dl4ss_mask_attn_align_loss (pass 0 COST, pass 1 GRAD; the same q / W1 / W2 / w3 / X / Y / strides / perm / s1 /
 * s2 / part_loss / part / mask_out / pred_out contract, K = 1..3, E = 50) with the two I/O forms the 'dot' kernels
 * have, as dl4ss_mask_attn_loss_ex / _bf16v:
 *   V or V_bf16 -- exactly one.  V_bf16: (B, T*F, E) raw bf16 words, contiguous, 4-B aligned, as the Linear's
 *     EPI_TANH_BF16 epilogue writes them; the kernel widens them to fp32 as it stages a tile, so every sum is the
 *     fp32 kernel's on those values: the COST pass's part_loss equals, bit for bit, that on the same values in fp32.
 *   dPre or dPre_bf16 -- in the GRAD pass exactly one.  dPre_bf16: a (B*T, dpre_bf16_ld) bf16 matrix, 4-B aligned,
 *     dpre_bf16_ld even and >= F*E: dPre of row (t, f) of utterance b, rounded to nearest even, at
 *     (b*T + t) * dpre_bf16_ld + f*E; the columns >= F*E of a row are never written.  fp32 dPre (B, T*F, E) may be
 *     V itself (fp32 V only: V_bf16 with fp32 dPre is refused, no step forms that pair).  The COST pass writes to
 *     neither; it may be handed the GRAD pass's pointers (dpre_bf16_ld is checked whenever dPre_bf16 is given).
 * hipErrorInvalidValue, before any launch and with nothing written, for: both or neither V pointer, both or
 * neither dPre pointer in the GRAD pass, dpre_bf16_ld < F*E or odd, a misaligned bf16 pointer, E != 50, K outside
 * 1..3, `part` missing or too small in the GRAD pass (part_floats < dl4ss_attn_align_part_floats(B, K, nblk)).
 * dl4ss_attn_align_finalize then forms dq and the three weight gradients from `part`, as after the fp32 entry. */
int dl4ss_mask_attn_align_loss_ex(int pass, int B, int K, int T, int F, int E, const float* V, const void* V_bf16,
                                  const float* q, const float* W1, const float* W2, const float* w3, const float* X,
                                  long long x_bstride, const float* Y, long long y_bstride, long long y_kstride,
                                  const int* perm, float s1, float s2, float* dPre, void* dPre_bf16,
                                  long long dpre_bf16_ld, float* part_loss, float* part, long long part_floats,
                                  float* mask_out, float* pred_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DL4SS_ALIGN_H */
