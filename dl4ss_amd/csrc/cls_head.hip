// Speaker-classifier head for gfx950: Linear + sigmoid on the time mean of the BiLSTM output, and the
// loss / backward of one training step.
//
// Replaces, in MIX_SPEECH_classifier (Torch_multi/test_multi_labels_speech.py:240-263) and its training
// loop (:389-445): self.Linear(mean_t h), F.sigmoid, nn.MultiLabelSoftMarginLoss (:397,437) and the
// autograd of the three.  The reference applies the loss to the sigmoid OUTPUT, not to the logits; that
// is kept.  With m = mean_t h (B, D = 2H), z = m W^T + b, p = sigmoid(z), labels y (B, C):
//
//   loss = -1/(B C) sum_{b,c} [ y log sigmoid(p) + (1 - y) log sigmoid(-p) ]
//   dz   = (sigmoid(p) - y) / (B C) * p (1 - p)
//   dW   = dz^T m      db = sum_b dz      dm = dz W
//   d(out)[b,t,:] = dm[b,:] / T            (the BPTT's dOut_bcast)
//
// C = N_lab is small (101) and D <= 1280: one wave per logit forward, one thread per output element
// backward.  Every sum runs in a fixed order (no float atomics): two launches agree bit for bit.
#include "common.h"

namespace {

constexpr int HEAD_NT = 256;

// z[b][c] = m[b] . W[c] + bias[c], p = sigmoid(z): wave w of block (b, c / 4) owns label c
__global__ __launch_bounds__(HEAD_NT) void cls_head_fwd_kernel(const float* __restrict__ m, const float* __restrict__ W,
                                                               const float* __restrict__ bias, int D, int C,
                                                               float* __restrict__ z, float* __restrict__ p) {
  const int b = blockIdx.x;
  const int c = blockIdx.y * (HEAD_NT / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= C) return;
  const float* mr = m + (long long)b * D;
  const float* wr = W + (long long)c * D;
  float acc = 0.f;
  for (int k = lane; k < D; k += 64) acc = fmaf(mr[k], wr[k], acc);
  acc = wave_sum(acc);
  if (lane == 0) {
    const float zz = acc + bias[c];
    z[(long long)b * C + c] = zz;
    p[(long long)b * C + c] = 1.0f / (1.0f + expf(-zz));
  }
}

// One workgroup: thread c walks its label's column over the batch rows in order (dz, db) and keeps its
// share of the loss; the shares are then added as a fixed pairwise tree.
__global__ __launch_bounds__(HEAD_NT) void cls_head_dz_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                              int B, int C, float* __restrict__ loss,
                                                              float* __restrict__ dz, float* __restrict__ db) {
  __shared__ float sl[HEAD_NT];
  const float inv = 1.0f / ((float)B * (float)C);
  float part = 0.f;
  for (int c = threadIdx.x; c < C; c += HEAD_NT) {
    float dbc = 0.f;
    for (int b = 0; b < B; ++b) {
      const float pp = p[(long long)b * C + c], yy = y[(long long)b * C + c];
      // log sigmoid(x) = -log1p(exp(-x)); x = +-p lies in [-1, 1]
      part += yy * -log1pf(expf(-pp)) + (1.0f - yy) * -log1pf(expf(pp));
      const float s = 1.0f / (1.0f + expf(-pp));
      const float g = (s - yy) * inv * (pp * (1.0f - pp));
      dz[(long long)b * C + c] = g;
      dbc += g;
    }
    db[c] = dbc;
  }
  sl[threadIdx.x] = part;
  __syncthreads();
  for (int w = HEAD_NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sl[threadIdx.x] += sl[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = -sl[0] * inv;
}

// blockIdx.y < C:  dW[c][k] = sum_b dz[b][c] m[b][k]           (rows in order)
// else b = y - C:  dmb[b][k] = (sum_c dz[b][c] W[c][k]) / T    (labels in order)
__global__ __launch_bounds__(HEAD_NT) void cls_head_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ m,
                                                               const float* __restrict__ W, int B, int D, int C,
                                                               float inv_T, float* __restrict__ dW,
                                                               float* __restrict__ dmb) {
  const int k = blockIdx.x * HEAD_NT + threadIdx.x;
  if (k >= D) return;
  if ((int)blockIdx.y < C) {
    const int c = blockIdx.y;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = fmaf(dz[(long long)b * C + c], m[(long long)b * D + k], acc);
    dW[(long long)c * D + k] = acc;
  } else {
    const int b = blockIdx.y - C;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) acc = fmaf(dz[(long long)b * C + c], W[(long long)c * D + k], acc);
    dmb[(long long)b * D + k] = acc * inv_T;
  }
}

}  // namespace

// m (B, D) the time mean of the top layer, W (C, D), b (C) -> logits z (B, C) and p = sigmoid(z)
DL4SS_API int dl4ss_cls_head_fwd(const float* m, const float* W, const float* b, int B, int D, int C, float* z,
                                 float* p, void* stream) {
  DL4SS_REQUIRE(m && W && b && z && p && B > 0 && D > 0 && C > 0 && B <= 65535);
  hipLaunchKernelGGL(cls_head_fwd_kernel, dim3(B, cdiv(C, HEAD_NT / 64)), dim3(HEAD_NT), 0, as_stream(stream), m, W, b,
                     D, C, z, p);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// p, y (B, C), m (B, D), W (C, D) -> loss (1), dz (B, C), dW (C, D), db (C), dOut_bcast (B, D) = dz W / T
DL4SS_API int dl4ss_cls_head_loss_bwd(const float* p, const float* y, const float* m, const float* W, int B, int D,
                                      int C, int T, float* loss, float* dz, float* dW, float* db, float* dOut_bcast,
                                      void* stream) {
  DL4SS_REQUIRE(p && y && m && W && loss && dz && dW && db && dOut_bcast);
  DL4SS_REQUIRE(B > 0 && D > 0 && C > 0 && T > 0 && (long long)B + C <= 65535);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(cls_head_dz_kernel, dim3(1), dim3(HEAD_NT), 0, st, p, y, B, C, loss, dz, db);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL(cls_head_bwd_kernel, dim3(cdiv(D, HEAD_NT), C + B), dim3(HEAD_NT), 0, st, dz, m, W, B, D, C,
                     1.0f / (float)T, dW, dOut_bcast);
  DL4SS_CHECK_LAUNCH();
  return 0;
}
