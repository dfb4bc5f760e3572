/* dl4ss_corpus.h -- C ABI of the device-resident corpus, an extension library of its own: libdl4ss_corpus.so,
 * built from csrc/corpus/ (libdl4ss_hip.so exports exactly what the headers directly under include/ declare, and
 * stays as it is).  The conventions are those of dl4ss_hip.h (int return = hipError_t, caller-owned device buffers,
 * `stream` a hipStream_t as void*, asynchronous, never allocates, no float atomics).
 *
 * The corpus is one flat pool of clips that stays on the device; a training step names its sources by clip id and
 * the mixing launch gathers, normalises, rotates, pads, scales and sums them -- what dl4ss_mix_sources_rot does
 * for an uploaded (B, K, N) array, with the per-clip statistics computed once per corpus instead of every step.
 *
 *   pool        int16 (dtype DL4SS_CORPUS_I16, sample = (float)q * 2^-15) or fp32 (DL4SS_CORPUS_F32) samples,
 *               16-B aligned; every clip starts 16-B aligned inside it
 *   offsets     (n_clips) long long, the first sample of each clip, in samples, a multiple of 8 (int16) / 4 (fp32)
 *   lengths     (n_clips) int, >= 1
 *   clip_stats  (n_clips, 2) float {mean, 1 / max|x - mean|} (0 for a constant clip), over the stored clip
 *
 * The builder of the pool guarantees offsets[c] + lengths[c] <= the pool's length and the alignment; the kernels
 * read a clip only through its table entries and never past lengths[c].
 *
 * Arithmetic (that of dl4ss_mix_sources_rot, bit for bit on the same samples): the statistics are 8 partials per
 * clip {fp64 sum, min, max} combined in ascending order, mean = float(sum / len), peak = max(mx - mean, mean - mn);
 * per element, with fp contraction off, g = gain * inv_peak, v = (x[(i + s) mod len] - mean) * g for i < len and 0
 * beyond, and the mixture is the fp32 sum over the sources in ascending order.
 */
#ifndef DL4SS_CORPUS_H
#define DL4SS_CORPUS_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DL4SS_CORPUS_I16 = 0,
  DL4SS_CORPUS_F32 = 1
};

/* clip_stats (n_clips, 2) = {mean, 1 / peak} of every clip.  ws: 16-B aligned workspace of 32 n_clips floats
 * (the 8 partials per clip), overwritten.  n_clips = 0: a no-op. */
int dl4ss_corpus_stats(const void* pool, int dtype, const long long* offsets, const int* lengths, int n_clips,
                       float* ws, float* clip_stats, void* stream);

/* One step's batch in one launch.  clips, shifts, gains: (B, Ks) device arrays (int, int, float); shifts may be
 * NULL (no rotation), else source j is rotated by shifts[j] modulo its clip's length (a negative shift wraps the
 * same way).  Sources 0..K-1 are written to out_src (B, K, N); sources K..Ks-1 are only summed into out_mix (B, N)
 * (a background clip that is no target).  1 <= K <= Ks <= 16, B <= 65535.  N >= every used clip's length: a longer
 * clip is cut at N, but its statistics stay those of the stored clip.  out_len (B, Ks) int, may be NULL: the
 * lengths used.  A clip id outside [0, n_clips) reads nothing: that source is silent (length 0) and bad[0] goes up
 * by one per such source (an integer atomic; the caller zeroes bad and reads it when it likes).  Every element of
 * out_src and out_mix is written.  B = 0: a no-op. */
int dl4ss_mix_corpus(const void* pool, int dtype, const long long* offsets, const int* lengths,
                     const float* clip_stats, int n_clips, const int* clips, const int* shifts, const float* gains,
                     int B, int K, int Ks, int N, float* out_src, float* out_mix, int* out_len, int* bad,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DL4SS_CORPUS_H */
