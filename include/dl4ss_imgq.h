/* dl4ss_imgq.h -- C ABI of the image-query encoder in libdl4ss_hip.so (csrc/imgq.hip): the second public
 * header, with the conventions of dl4ss_hip.h (int return = hipError_t, caller-owned fp32 device buffers,
 * `stream` a hipStream_t as void*, asynchronous, never allocates).
 *
 * The encoder is the small CNN that names the target by a picture
 * (Multi_modal/software/DL4SS_Keras/nnet.py:70-89), torch conventions throughout (cross-correlation, NCHW
 * flatten order, floor pooling):
 *
 *   images (n, h, w), one channel
 *   conv1  4 filters 5x5, valid, + bias, ReLU, max-pool 2x2   -> (4, h1, w1),  h1 = (h - 4) / 2
 *   conv2  8 filters 3x3, valid, + bias, ReLU, max-pool 2x2   -> (8, h2, w2),  h2 = (h1 - 2) / 2
 *   conv3 16 filters 3x3, valid, + bias, ReLU, max-pool 2x2   -> (16, h3, w3), h3 = (h2 - 2) / 2
 *   dense  flatten (C, H, W) -> Linear(D = 16 h3 w3, E) + bias, no activation -> vec (n, E)
 *
 * (integer division: a trailing odd row / column of a pooling input is dropped; w likewise.)
 *
 * Parameter block `params`, P = dl4ss_imgq_param_count(h, w, E) floats, every tensor in torch's layout:
 *   [0, 100) conv1.weight (4, 1, 5, 5)    [100, 104) conv1.bias
 *   [104, 392) conv2.weight (8, 4, 3, 3)  [392, 400) conv2.bias
 *   [400, 1552) conv3.weight (16, 8, 3, 3) [1552, 1568) conv3.bias
 *   [1568, 1568 + E D) dense.weight (E, D)  then dense.bias (E)
 * P = 2418 at 28 x 28, E = 50.
 *
 * Gradient rules (torch's): ReLU passes nothing at a pre-activation <= 0; a pooling window sends its gradient
 * to its first maximum in row-major window order (over a flat background every pre-activation of a window
 * equals the bias, so ties are the normal case).
 *
 * Image sizes: DL4SS_IMGQ_MIN_HW <= h, w <= DL4SS_IMGQ_MAX_HW (below the minimum a stage keeps no pooled
 * cell; the maximum is what the kernels' LDS plan -- the image, the three pooled maps with their arg-max
 * codes, the three gradient maps and the convolution parameters, 42 KB at 48 x 48 -- is sized for).
 * 1 <= E <= DL4SS_IMGQ_MAX_E and n <= DL4SS_IMGQ_MAX_N (the speaker memory's limits).
 */
#ifndef DL4SS_IMGQ_H
#define DL4SS_IMGQ_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DL4SS_IMGQ_MIN_HW = 24,
  DL4SS_IMGQ_MAX_HW = 48,
  DL4SS_IMGQ_MAX_E = 128,
  DL4SS_IMGQ_MAX_N = 1024,
  DL4SS_IMGQ_CONV_PARAMS = 1568, /* floats in front of dense.weight */
  DL4SS_IMGQ_OFF_W1 = 0,
  DL4SS_IMGQ_OFF_B1 = 100,
  DL4SS_IMGQ_OFF_W2 = 104,
  DL4SS_IMGQ_OFF_B2 = 392,
  DL4SS_IMGQ_OFF_W3 = 400,
  DL4SS_IMGQ_OFF_B3 = 1552,
  DL4SS_IMGQ_OFF_WD = 1568
};

/* P of the parameter block, or -1 for an (h, w, E) outside the limits. */
long long dl4ss_imgq_param_count(int h, int w, int E);
/* D = 16 h3 w3, the dense layer's input width, or -1. */
long long dl4ss_imgq_dense_in(int h, int w);

/* vec (n, E) = the encoder over images (n, h, w).  One workgroup per image; every element of vec written.
 * n = 0: a no-op.  vec must not alias images or params. */
int dl4ss_imgq_fwd(const float* images, const float* params, int n, int h, int w, int E, float* vec, void* stream);

/* dpart (n, ld): row i = image i's own parameter gradient for the upstream gradient dvec (n, E), in the
 * parameter block's layout, columns [P, ld) zero; every element written, no atomics.  The forward is
 * recomputed from the image: nothing is kept between dl4ss_imgq_fwd and this call.  The batch gradient is the
 * column sum of dpart (dl4ss_imgq_reduce).  ld >= P; dpart_floats (the buffer's
 * length) >= n * ld.  n = 0: a no-op.  dpart must not alias images, dvec or params. */
int dl4ss_imgq_bwd(const float* images, const float* dvec, const float* params, int n, int h, int w, int E,
                   float* dpart, long long ld, long long dpart_floats, void* stream);

/* out (ld) = the column sums of dpart (n, ld), every element written, no atomics, the same bits for the same n.
 * Order: pairwise.  Rows are taken in ascending order; whenever two sums of 2^l consecutive rows exist they are
 * added, earlier + later; the sums left at the end (one per set bit of n) are folded from the latest rows back:
 * total = sum(earlier block) + total.  (dl4ss_vp_colsum has the same contract with a serial order, whose
 * rounding error grows with n; this one's grows with log2 n.)  n = 0: a no-op (out untouched).  out must not
 * alias dpart. */
int dl4ss_imgq_reduce(const float* dpart, int n, long long ld, float* out, void* stream);

/* The image-query step's loss guard: status[0] |= 2 when loss[0] is not finite, so that every guarded Adam
 * and the memory store behind it refuse the step (status[0] bit 0 stays the recurrences' time-out flag). */
int dl4ss_imgq_guard(const float* loss, int* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DL4SS_IMGQ_H */
