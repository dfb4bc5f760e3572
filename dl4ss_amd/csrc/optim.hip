// The Keras trees' optimizer (DL4SS_Keras/nnet.py:23,113: Nadam(clipnorm=200)): Keras 1's Nadam and its clipnorm
// rule as further instantiations of the one guarded update kernel (update.h), behind the entry points of
// include/dl4ss_optim.h.  A streaming kernel: seven fp32 streams in 16-B accesses (and the bf16 shadows), a few
// FMAs, a division and a square root per element; the clip adds a <= 32 KB read of fp64 partials per block.
#define DL4SS_UPDATE_ALL
#include "update.h"

#include "../../include/dl4ss_optim.h"

static_assert(DL4SS_CLIP_MAX_PARTS == CLIP_MAX_PARTS && DL4SS_STATUS_NONFINITE_GRAD == STATUS_NONFINITE_GRAD,
              "dl4ss_optim.h and update.h disagree");

namespace {
// the clip's arguments, checked; clip: CLIP_NONE (part NULL) or the rule's instantiation
int clip_args(ClipArgs& cl, int& clip, const double* part, int n_part, int clip_rule, float max_norm, float* gnorm,
              int* nonfinite, int nonfinite_sticky, int* status) {
  clip = CLIP_NONE;
  if (!part) return 0;
  DL4SS_REQUIRE(n_part >= 1 && n_part <= CLIP_MAX_PARTS && ((uintptr_t)part & 7) == 0);
  DL4SS_REQUIRE((clip_rule == DL4SS_CLIP_TORCH || clip_rule == DL4SS_CLIP_KERAS) && max_norm > 0.f && nonfinite);
  DL4SS_REQUIRE(!nonfinite_sticky || status);
  cl = ClipArgs{part, n_part, max_norm, gnorm, nonfinite, nonfinite_sticky ? 1 : 0};
  clip = clip_rule == DL4SS_CLIP_KERAS ? CLIP_KERAS : CLIP_TORCH;
  return 0;
}
}  // namespace

DL4SS_API int dl4ss_nadam(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                          float beta2, float eps, int step, double mu, double mu_next, double mu_prod, int* status,
                          const float* dp_flag, float gscale, float* loss, int nseg, const long long* seg_off,
                          const int* seg_rows, const int* seg_cols, void* const* seg_y, const long long* seg_ldy,
                          const double* part, int n_part, int clip_rule, float max_norm, float* gnorm,
                          int* nonfinite, int nonfinite_sticky, void* stream) {
  // mu_prod = 0 is a valid limit: the product of ~0.5s underflows in double after ~900 updates at beta1 < 0.87 or
  // schedule_decay 0, and a1 = lr (1 - mu), a2 = lr mu_next there
  DL4SS_REQUIRE(step >= 1 && mu > 0.0 && mu < 1.0 && mu_next > 0.0 && mu_next < 1.0 && mu_prod >= 0.0 && mu_prod < 1.0);
  ShadowSegs sh{};
  if (int rc = shadow_segs(sh, n, nseg, seg_off, seg_rows, seg_cols, seg_y, seg_ldy)) return rc;
  ClipArgs cl{};
  int clip;
  if (int rc = clip_args(cl, clip, part, n_part, clip_rule, max_norm, gnorm, nonfinite, nonfinite_sticky, status))
    return rc;
  // in double, each rounded once to fp32 (Keras carries m_schedule in fp32)
  UpdateScalars us{UPD_NADAM, 1.f, (float)sqrt(1.0 - pow((double)beta2, (double)step)),
                   (float)((double)lr * (1.0 - mu) / (1.0 - mu_prod)),
                   (float)((double)lr * mu_next / (1.0 - mu_prod * mu_next))};
  return update_launch(us, clip, p, g, m, v, n, lr, beta1, beta2, eps, status, status ? status + 1 : nullptr, dp_flag,
                       gscale, loss, stream, &sh, clip != CLIP_NONE ? &cl : nullptr);
}

DL4SS_API int dl4ss_adam_clipped_ex(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                                    float beta2, float eps, int step, int* status, const float* dp_flag,
                                    float gscale, float* loss, int nseg, const long long* seg_off,
                                    const int* seg_rows, const int* seg_cols, void* const* seg_y,
                                    const long long* seg_ldy, const double* part, int n_part, int clip_rule,
                                    float max_norm, float* gnorm, int* nonfinite, int nonfinite_sticky,
                                    void* stream) {
  DL4SS_REQUIRE(step >= 1);
  ShadowSegs sh{};
  if (int rc = shadow_segs(sh, n, nseg, seg_off, seg_rows, seg_cols, seg_y, seg_ldy)) return rc;
  ClipArgs cl{};
  int clip;
  if (int rc = clip_args(cl, clip, part, n_part, clip_rule, max_norm, gnorm, nonfinite, nonfinite_sticky, status))
    return rc;
  return update_launch(adam_scalars(beta1, beta2, step), clip, p, g, m, v, n, lr, beta1, beta2, eps, status,
                       status ? status + 1 : nullptr, dp_flag, gscale, loss, stream, &sh,
                       clip != CLIP_NONE ? &cl : nullptr);
}
