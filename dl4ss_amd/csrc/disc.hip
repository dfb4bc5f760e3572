// The adversarial Discriminator for gfx950: three Conv2d(., 64, 3x3, stride 2, 'valid') + ReLU on the
// (N, T, F) magnitude maps, Linear(64 H3 W3, 1) + sigmoid, and the backward of all four.
//
// Replaces, in the reference's Discriminator (TDAA_beta/main_run_sstune_dis.py:318-336, the same class in
// main_run_sstune_EvalVer.py:328-346) and its use (dis.py:615-647): nn.Conv2d x3, F.relu, nn.Linear,
// F.sigmoid, nn.MSELoss against 1 / 0 and the autograd of all of them.
//
// Layouts.  Activations are channels-last (N, H, W, 64): the implicit-GEMM K index (kh, kw, cin) has 64
// contiguous channels per tap.  Parameters stay in the reference's layouts: cnn*.weight (64, Cin, 3, 3) and
// final.weight (1, 64 H3 W3) flattened (c, h, w); the kernels do the index mapping, nothing is repacked in
// global memory.
//
// Precisions (ops.PREC).  fp32: activations fp32, v_mfma_f32_32x32x2_f32 (exact fp32 products).  bf16:
// activations y1..y3 and the activation gradients are stored as bf16, the filter banks are rounded to bf16
// while staged into LDS, forward and dX run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; conv1
// (K = 9) and every parameter gradient accumulate in fp32 from the stored operands (dW runs the fp32 MFMA
// on the bf16 values, which are exact in fp32).
//
// No float atomics: every sum runs in a fixed order, two launches agree bit for bit.
#include "common.h"

#include <type_traits>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short bf16_t;

constexpr int CH = 64;       // channels of every conv layer
constexpr int NT = 256;      // threads per workgroup (4 waves)
constexpr int BM = 128;      // igemm rows (positions) per workgroup
constexpr int LDF = 65;      // fp32 LDS row stride (floats): odd, fragment reads conflict-free
constexpr int LDH = 72;      // bf16 LDS row stride (elements): 144 B rows keep ds_read_b128 aligned
constexpr int DW_BK = 64;    // positions per dW reduction tile
constexpr int DW_CHUNK = 256;   // target positions per dW split
constexpr int DW_MAX_SPLIT = 128;
constexpr int C1_ROWS = 10;  // conv1 partial row: 9 taps + bias
constexpr int C1_CHUNK = 512;   // target positions per conv1 dW split (its partials are 640 floats)
constexpr int C1_MAX_SPLIT = 1024;

__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return __uint_as_float((unsigned)*p << 16); }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { *p = (bf16_t)bf16_bits_rne(v); }

// 8 consecutive channels (the row starts are 128 / 256 B aligned)
__device__ __forceinline__ void ld8(const float* p, float v[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void ld8(const bf16_t* p, float v[8]) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xFFFF0000u);
  v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xFFFF0000u);
  v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xFFFF0000u);
  v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xFFFF0000u);
}

static inline int out_dim(int in) { return (in - 3) / 2 + 1; }

struct Geom {
  int N, Hin, Win, Hout, Wout;
};

// ------------------------------------------------------------------------------------------------ conv1
// x (N, T, F) fp32, w (64, 1, 3, 3), b (64) -> y1 (N, H1, W1, 64) = relu(conv).  Thread = (position, channel).
template <typename T>
__global__ __launch_bounds__(NT) void conv1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ b, Geom g, T* __restrict__ y) {
  const int co = threadIdx.x & 63, q = threadIdx.x >> 6;
  float wv[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wv[t] = w[co * 9 + t];
  const float bv = b[co];
  const long long P = (long long)g.N * g.Hout * g.Wout;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long p = (long long)blockIdx.x * 16 + i * 4 + q;
    if (p >= P) continue;
    const unsigned pu = (unsigned)p, row = pu / (unsigned)g.Wout;  // P < 2^31 (geom_ok)
    const int ow = (int)(pu - row * g.Wout), oh = (int)(row % (unsigned)g.Hout), n = (int)(row / (unsigned)g.Hout);
    const float* xp = x + ((long long)n * g.Hin + 2 * oh) * g.Win + 2 * ow;
    float acc = bv;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) acc = fmaf(xp[(long long)kh * g.Win + kw], wv[kh * 3 + kw], acc);
    st1(y + p * CH + co, fmaxf(acc, 0.f));
  }
}

// dx[n, t, f] = sum_{taps} sum_co (dy1 * [y1 > 0])[n, oh, ow, co] w[co, tap].  A workgroup owns a tile of
// DX_TH x DX_TW half-resolution positions (a, b) = (t >> 1, f >> 1), i.e. 2 DX_TH x 2 DX_TW pixels.
// Phase 1: for the tile's output positions and a one-position halo above / left (tap 2 of an even index
// reaches output a - 1), col[pos][tap] = sum_co g[pos][co] w[co][tap] -- 16 lanes per position, 4 channels
// each (dy1 and y1 are read once, coalesced), then a fixed butterfly over the 16 lanes; positions outside
// the output get zeros.  Phase 2: every pixel gathers its 4 / 2 / 2 / 1 taps from col in LDS; a pixel no
// window covers sums zeros only.
constexpr int DX_TH = 4, DX_TW = 66, DX_POS = (DX_TH + 1) * (DX_TW + 1);

__device__ __forceinline__ void ld4(const float* p, float v[4]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void ld4(const bf16_t* p, float v[4]) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xFFFF0000u);
  v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xFFFF0000u);
}

template <typename T>
__global__ __launch_bounds__(NT) void conv1_dx_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                                      const float* __restrict__ w, Geom g, int tilesH, int tilesW,
                                                      float* __restrict__ dx) {
  __shared__ float col[DX_POS * 9];
  const int tid = threadIdx.x, c4 = tid & 15, q = tid >> 4;
  const int tw_ = blockIdx.x % tilesW, th_ = (blockIdx.x / tilesW) % tilesH, n = blockIdx.x / (tilesW * tilesH);
  const int a0 = th_ * DX_TH, b0 = tw_ * DX_TW;
  float wv[4][9];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[j][t] = w[(c4 * 4 + j) * 9 + t];
  for (int pp = q; pp < DX_POS; pp += NT / 16) {
    const int oh = a0 - 1 + pp / (DX_TW + 1), ow = b0 - 1 + pp % (DX_TW + 1);
    float s[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) s[t] = 0.f;
    if (oh >= 0 && oh < g.Hout && ow >= 0 && ow < g.Wout) {
      const long long o = (((long long)n * g.Hout + oh) * g.Wout + ow) * CH + c4 * 4;
      float gv[4], yv[4];
      ld4(dy + o, gv);
      ld4(y + o, yv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = yv[j] > 0.f ? gv[j] : 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) s[t] = fmaf(v, wv[j][t], s[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s[t] += __shfl_xor(s[t], o, 16);
    }
    if (c4 == 0) {
#pragma unroll
      for (int t = 0; t < 9; ++t) col[pp * 9 + t] = s[t];
    }
  }
  __syncthreads();
  for (int i = tid; i < 4 * DX_TH * DX_TW; i += NT) {
    const int lr = i / (2 * DX_TW), lc = i % (2 * DX_TW);
    const int ih = 2 * a0 + lr, iw = 2 * b0 + lc;
    if (ih >= g.Hin || iw >= g.Win) continue;
    const int ph = lr & 1, pw = lc & 1;
    float acc = 0.f;
    for (int th = 0; th < (ph ? 1 : 2); ++th) {
      const int kh = ph ? 1 : 2 * th, r = (lr >> 1) - th + 1;   // col row 0 is output row a0 - 1
      for (int tw = 0; tw < (pw ? 1 : 2); ++tw) {
        const int kw = pw ? 1 : 2 * tw, c = (lc >> 1) - tw + 1;
        acc += col[(r * (DX_TW + 1) + c) * 9 + kh * 3 + kw];
      }
    }
    dx[((long long)n * g.Hin + ih) * g.Win + iw] = acc;
  }
}

// Split s of the positions: part[s][co][0..8] = sum_p g[p][co] x[tap of p], part[s][co][9] = sum_p g[p][co]
template <typename T>
__global__ __launch_bounds__(NT) void conv1_dw_part_kernel(const float* __restrict__ x, const T* __restrict__ dy,
                                                           const T* __restrict__ y, Geom g, long long chunk,
                                                           float* __restrict__ part) {
  __shared__ float red[4][CH][C1_ROWS + 1];
  const int co = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long long P = (long long)g.N * g.Hout * g.Wout;
  const long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
  float acc[C1_ROWS];
#pragma unroll
  for (int t = 0; t < C1_ROWS; ++t) acc[t] = 0.f;
  for (long long p = p0 + q; p < p1; p += 4) {
    const float v = ld1(y + p * CH + co) > 0.f ? ld1(dy + p * CH + co) : 0.f;
    const unsigned pu = (unsigned)p, row = pu / (unsigned)g.Wout;  // P < 2^31 (geom_ok)
    const int ow = (int)(pu - row * g.Wout), oh = (int)(row % (unsigned)g.Hout), n = (int)(row / (unsigned)g.Hout);
    const float* xp = x + ((long long)n * g.Hin + 2 * oh) * g.Win + 2 * ow;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) acc[kh * 3 + kw] = fmaf(v, xp[(long long)kh * g.Win + kw], acc[kh * 3 + kw]);
    acc[9] += v;
  }
#pragma unroll
  for (int t = 0; t < C1_ROWS; ++t) red[q][co][t] = acc[t];
  __syncthreads();
  if (q == 0) {
#pragma unroll
    for (int t = 0; t < C1_ROWS; ++t)
      part[((long long)blockIdx.x * CH + co) * C1_ROWS + t] = ((red[0][co][t] + red[1][co][t]) + red[2][co][t]) + red[3][co][t];
  }
}

// --------------------------------------------------------------------------------- 64 -> 64 implicit GEMM
// One kernel for the forward and the input gradient; rows are positions, the K loop walks the taps (64
// channels each), the 64 output columns are channels.  128 rows per workgroup, wave w owns rows
// 32 w .. 32 w + 31 as two 32x32 accumulators.  The A rows are gathered per tap from the channels-last
// activation (no im2col buffer); the tap's 64 x 64 filter slice is staged from the (co, ci, kh, kw) bank.
//
//   DX = false: src = X (N, Hin, Win, 64), dst = Y (N, Hout, Wout, 64) = relu(conv + bias), 9 taps.
//   DX = true : src = dY, gate = Y (N, Hout, Wout, 64), dst = dX (N, Hin, Win, 64).  blockIdx.y is the
//               parity class (ih & 1, iw & 1) of the input position: an even index is reached by taps
//               {0, 2}, an odd one by tap {1}, so the classes sum 4 / 2 / 2 / 1 taps.  Position (2a + ph)
//               takes tap th from output row a - th; rows outside [0, Hout) contribute zeros, which also
//               writes the exact zeros of a last row / column that no window covers.
template <typename T, bool DX>
__global__ __launch_bounds__(NT) void conv64_igemm_kernel(const T* __restrict__ src, const T* __restrict__ gate,
                                                          const float* __restrict__ W, const float* __restrict__ bias,
                                                          Geom g, T* __restrict__ dst) {
  constexpr bool BF = !std::is_same<T, float>::value;
  constexpr int LDA = BF ? LDH : LDF;
  __shared__ __attribute__((aligned(16))) T sA[BM * LDA];
  __shared__ __attribute__((aligned(16))) T sB[CH * LDA];
  __shared__ int sBase[BM], sRa[BM], sRb[BM], sDst[BM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
  int ph = 0, pw = 0, Ha = g.Hout, Wa = g.Wout;
  if (DX) {
    ph = blockIdx.y >> 1;
    pw = blockIdx.y & 1;
    Ha = (g.Hin - ph + 1) >> 1;
    Wa = (g.Win - pw + 1) >> 1;
  }
  const long long M = (long long)g.N * Ha * Wa;
  const long long m0 = (long long)blockIdx.x * BM;
  if (m0 >= M) return;  // a smaller parity class: uniform over the workgroup, before any barrier

  if (tid < BM) {
    const long long m = m0 + tid;
    int base = 0, ra = -(1 << 20), rb = 0, d = -1;
    if (m < M) {
      const int b = (int)(m % Wa), a = (int)((m / Wa) % Ha), n = (int)(m / ((long long)Wa * Ha));
      ra = a;
      rb = b;
      if (DX) {
        base = (n * g.Hout + a) * g.Wout + b;
        d = (n * g.Hin + 2 * a + ph) * g.Win + 2 * b + pw;
      } else {
        base = (n * g.Hin + 2 * a) * g.Win + 2 * b;
        d = (int)m;
      }
    }
    sBase[tid] = base;
    sRa[tid] = ra;
    sRb[tid] = rb;
    sDst[tid] = d;
  }

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int nth = DX ? (ph ? 1 : 2) : 3, ntw = DX ? (pw ? 1 : 2) : 3;
  for (int tt = 0; tt < nth * ntw; ++tt) {
    const int th = tt / ntw, tw = tt % ntw;
    const int kh = DX ? (ph ? 1 : 2 * th) : th, kw = DX ? (pw ? 1 : 2 * tw) : tw;
    __syncthreads();  // the row table is written / the previous tap's fragments are read
    // A: 128 rows x 8 chunks of 8 channels
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (tid >> 3) + 32 * i, c8 = (tid & 7) * 8;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
      bool ok;
      long long row;
      if (DX) {
        const int oh = sRa[r] - th, ow = sRb[r] - tw;
        ok = oh >= 0 && oh < g.Hout && ow >= 0 && ow < g.Wout;
        row = (long long)sBase[r] - th * g.Wout - tw;
      } else {
        ok = sRa[r] >= 0;
        row = (long long)sBase[r] + kh * g.Win + kw;
      }
      if (ok) {
        ld8(src + row * CH + c8, v);
        if (DX) {
          float gt[8];
          ld8(gate + row * CH + c8, gt);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = gt[j] > 0.f ? v[j] : 0.f;
        }
      }
      if (BF) {
        // the values are bf16 already (or zero): the truncation is exact
        uint4 u;
        u.x = (__float_as_uint(v[0]) >> 16) | (__float_as_uint(v[1]) & 0xFFFF0000u);
        u.y = (__float_as_uint(v[2]) >> 16) | (__float_as_uint(v[3]) & 0xFFFF0000u);
        u.z = (__float_as_uint(v[4]) >> 16) | (__float_as_uint(v[5]) & 0xFFFF0000u);
        u.w = (__float_as_uint(v[6]) >> 16) | (__float_as_uint(v[7]) & 0xFFFF0000u);
        *reinterpret_cast<uint4*>(&sA[r * LDA + c8]) = u;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) st1(&sA[r * LDA + c8 + j], v[j]);
      }
    }
    // B: the tap's slice W[co][ci][kh][kw]; k = ci, n = co forward, k = co, n = ci for dX.
    // fp32 image [k][n], bf16 image [n][k] (rounded to bf16 here)
    for (int e = tid; e < CH * CH; e += NT) {
      const int co = e >> 6, ci = e & 63;
      const float wv = W[(long long)e * 9 + kh * 3 + kw];
      const int k = DX ? co : ci, n = DX ? ci : co;
      st1(&sB[BF ? n * LDA + k : k * LDA + n], wv);
    }
    __syncthreads();
    if (BF) {
#pragma unroll
      for (int kk = 0; kk < CH; kk += 16) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(&sA[(wave * 32 + fr) * LDA + kk + 8 * fh]);
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(&sB[fr * LDA + kk + 8 * fh]);
        const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(&sB[(32 + fr) * LDA + kk + 8 * fh]);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b1, acc[1], 0, 0, 0);
      }
    } else {
      const float* fA = reinterpret_cast<const float*>(sA);
      const float* fB = reinterpret_cast<const float*>(sB);
#pragma unroll 8
      for (int kk = 0; kk < CH; kk += 2) {
        const float a = fA[(wave * 32 + fr) * LDA + kk + fh];
        const float b0 = fB[(kk + fh) * LDA + fr];
        const float b1 = fB[(kk + fh) * LDA + 32 + fr];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
      }
    }
  }

  // epilogue: acc[j][r] is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column 32 j + (lane & 31)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = 32 * j + fr;
    const float bv = DX ? 0.f : bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      const int d = sDst[row];
      if (d < 0) continue;
      float v = acc[j][r];
      if (!DX) v = fmaxf(v + bv, 0.f);
      st1(dst + (long long)d * CH + col, v);
    }
  }
}

// dW of a 64 -> 64 layer: M = 64 (co), N = 9 x 64 (tap, ci), reduced over the positions.  Workgroup
// (split s, tap): its positions in tiles of 64, G = dY * [Y > 0] and the tap's X rows staged as fp32,
// wave w owns the 32 x 32 block (co half w >> 1, ci half w & 1) on the fp32 MFMA.  The tap-0 workgroup of a
// split also sums G's columns (db) row by row.  part [S][9 x 64 co x 64 ci + 64].
template <typename T>
__global__ __launch_bounds__(NT) void conv64_dw_part_kernel(const T* __restrict__ X, const T* __restrict__ dY,
                                                            const T* __restrict__ Y, Geom g, long long chunk,
                                                            float* __restrict__ part) {
  __shared__ float sG[DW_BK * LDF];
  __shared__ float sX[DW_BK * LDF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
  const int tap = blockIdx.y, kh = tap / 3, kw = tap % 3;
  const long long P = (long long)g.N * g.Hout * g.Wout;
  const long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
  const int co0 = (wave >> 1) * 32, ci0 = (wave & 1) * 32;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float dbacc = 0.f;
  for (long long pt = p0; pt < p1; pt += DW_BK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (tid >> 3) + 32 * i, c8 = (tid & 7) * 8;
      const long long p = pt + r;
      float gv[8], xv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) gv[j] = xv[j] = 0.f;
      if (p < p1) {
        float yv[8];
        ld8(dY + p * CH + c8, gv);
        ld8(Y + p * CH + c8, yv);
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] = yv[j] > 0.f ? gv[j] : 0.f;
        const unsigned pu = (unsigned)p, row = pu / (unsigned)g.Wout;  // P < 2^31 (geom_ok)
        const int ow = (int)(pu - row * g.Wout), oh = (int)(row % (unsigned)g.Hout), n = (int)(row / (unsigned)g.Hout);
        ld8(X + (((long long)n * g.Hin + 2 * oh + kh) * g.Win + 2 * ow + kw) * CH + c8, xv);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sG[r * LDF + c8 + j] = gv[j];
        sX[r * LDF + c8 + j] = xv[j];
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < DW_BK; kk += 2) {
      const float a = sG[(kk + fh) * LDF + co0 + fr];
      const float b = sX[(kk + fh) * LDF + ci0 + fr];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    if (tap == 0 && tid < CH)
      for (int k = 0; k < DW_BK; ++k) dbacc += sG[k * LDF + tid];
  }
  float* ps = part + (long long)blockIdx.x * (9 * CH * CH + CH);  // this split: [9][64 co][64 ci], then [64]
  float* pw = ps + tap * CH * CH;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
    pw[co * CH + ci0 + fr] = acc[r];
  }
  if (tap == 0 && tid < CH) ps[9 * CH * CH + tid] = dbacc;
}

// The splits' partials -> dw / db.  part is [S][E]: E = 64 x 10 (co, 9 taps + bias) for conv1, E = 9 x 64 x 64
// (tap, co, ci) + 64 (bias) for a 64 -> 64 layer.  Thread (j, el) of a workgroup adds the splits j, j + 16, ...
// of output element 16 blockIdx.x + el in order, thread (0, el) then adds the 16 sums in order: a fixed
// two-level order with 16-fold shorter serial chains than one thread per element.
template <bool C1>
__global__ __launch_bounds__(NT) void dw_combine_kernel(const float* __restrict__ part, int S, float* __restrict__ dw,
                                                        float* __restrict__ db) {
  constexpr int E = C1 ? CH * C1_ROWS : 9 * CH * CH + CH;
  __shared__ float red[16][17];
  const int el = threadIdx.x & 15, j = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  float acc = 0.f;
  if (e < E)
    for (int s = j; s < S; s += 16) acc += part[(long long)s * E + e];
  red[j][el] = acc;
  __syncthreads();
  if (j != 0 || e >= E) return;
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) t += red[k][el];
  if (C1) {
    const int co = e / C1_ROWS, tt = e % C1_ROWS;
    if (tt < 9) dw[co * 9 + tt] = t;
    else db[co] = t;
  } else if (e < 9 * CH * CH) {
    const int tap = e / (CH * CH), co = (e / CH) % CH, ci = e % CH;
    dw[(co * CH + ci) * 9 + tap] = t;
  } else {
    db[e - 9 * CH * CH] = t;
  }
}

// --------------------------------------------------------------------------------------------------- head
// z[n] = sum_{h,w,c} y3[n, h, w, c] wf[c H3 W3 + h W3 + w] + b, score = sigmoid(z).  One workgroup per map:
// strided partial sums, then a fixed pairwise tree.
template <typename T>
__global__ __launch_bounds__(NT) void head_fwd_kernel(const T* __restrict__ y3, const float* __restrict__ wf,
                                                      const float* __restrict__ bf, int HW, float* __restrict__ z,
                                                      float* __restrict__ score) {
  __shared__ float red[NT];
  const int n = blockIdx.x, L = HW * CH;
  const T* yr = y3 + (long long)n * L;
  float acc = 0.f;
  for (int q = threadIdx.x; q < L; q += NT) acc = fmaf(ld1(yr + q), wf[(q & 63) * HW + (q >> 6)], acc);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float zz = red[0] + bf[0];
    z[n] = zz;
    score[n] = 1.0f / (1.0f + expf(-zz));
  }
}

// dz[n] = dL/dscore[n] * s (1 - s), with dL/dscore given or that of loss = mean_n (s - target)^2;
// db = sum_n dz in map order.  One thread: N is the number of maps.
__global__ void head_dz_kernel(const float* __restrict__ score, const float* __restrict__ dscore, float target, int N,
                               float* __restrict__ loss, float* __restrict__ dz, float* __restrict__ db) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float l = 0.f, dbs = 0.f;
  const float inv = 1.0f / (float)N;
  for (int n = 0; n < N; ++n) {
    const float s = score[n], e = s - target;
    const float gs = dscore ? dscore[n] : 2.0f * e * inv;
    const float d = gs * (s * (1.0f - s));
    l = fmaf(e, e, l);
    dz[n] = d;
    dbs += d;
  }
  db[0] = dbs;
  if (loss) loss[0] = l * inv;
}

// The adversarial step's three loss heads (dis.py:622-624,642) over the scores [true (N); fake (N)]:
// loss[0] = L_dt = mean (s_true - 1)^2, loss[1] = L_df = mean s_fake^2, loss[2] = L_adv = mean (s_fake - 1)^2
// (unweighted), ds_dis (2N) = d(L_dt + L_df)/dscore = 2 (s - 1) / N | 2 s / N, ds_adv (N) =
// lambda 2 (s_fake - 1) / N.  One thread, maps in order, the sums in fp64: N is the number of maps.
__global__ void adv_heads_kernel(const float* __restrict__ score, int N, float lambda, float* __restrict__ loss,
                                 float* __restrict__ ds_dis, float* __restrict__ ds_adv) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float inv = 1.0f / (float)N;
  double lt = 0.0, lf = 0.0, la = 0.0;
  for (int n = 0; n < N; ++n) {
    const float st = score[n], sf = score[N + n];
    const float et = st - 1.0f, ea = sf - 1.0f;
    lt += (double)et * et;
    lf += (double)sf * sf;
    la += (double)ea * ea;
    ds_dis[n] = 2.0f * et * inv;
    ds_dis[N + n] = 2.0f * sf * inv;
    ds_adv[n] = lambda * (2.0f * ea * inv);
  }
  loss[0] = (float)(lt / N);
  loss[1] = (float)(lf / N);
  loss[2] = (float)(la / N);
}

// dwf[c, h, w] = sum_n dz[n] y3[n, h, w, c] (maps in order), dy3[n, h, w, c] = dz[n] wf[c, h, w]
template <typename T>
__global__ __launch_bounds__(NT) void head_bwd_kernel(const T* __restrict__ y3, const float* __restrict__ wf,
                                                      const float* __restrict__ dz, int N, int HW,
                                                      float* __restrict__ dwf, T* __restrict__ dy3) {
  const int L = HW * CH;
  const int q = blockIdx.x * NT + threadIdx.x;
  if (q >= L) return;
  const int o = (q & 63) * HW + (q >> 6);
  const float wv = wf[o];
  float acc = 0.f;
  for (int n = 0; n < N; ++n) {
    const float d = dz[n];
    acc = fmaf(d, ld1(y3 + (long long)n * L + q), acc);
    st1(dy3 + (long long)n * L + q, d * wv);
  }
  dwf[o] = acc;
}

// ------------------------------------------------------------------------------------------ host helpers
bool geom_ok(int N, int Hin, int Win) {
  return N > 0 && Hin >= 3 && Win >= 3 && (long long)N * Hin * Win < (1LL << 31);  // row indices are ints
}

Geom make_geom(int N, int Hin, int Win) { return Geom{N, Hin, Win, out_dim(Hin), out_dim(Win)}; }

int dw_splits(long long P, int chunk = DW_CHUNK, int max_split = DW_MAX_SPLIT) {
  long long s = (P + chunk - 1) / chunk;
  return (int)(s < 1 ? 1 : (s > max_split ? max_split : s));
}

// positions per split, a multiple of the reduction tile
long long dw_chunk(long long P, int S) {
  const long long c = (P + S - 1) / S;
  return (c + DW_BK - 1) / DW_BK * DW_BK;
}

long long conv64_ws_floats(long long P) { return (long long)dw_splits(P) * (9 * CH * CH + CH); }
long long conv1_ws_floats(long long P) { return (long long)dw_splits(P, C1_CHUNK, C1_MAX_SPLIT) * CH * C1_ROWS; }

template <typename T>
int conv64_bwd_t(const T* x, const T* y, const T* dy, const float* w, Geom g, T* dx, float* dw, float* db, float* ws,
                 hipStream_t st) {
  const long long P = (long long)g.N * g.Hout * g.Wout;
  const int S = dw_splits(P);
  hipLaunchKernelGGL(conv64_dw_part_kernel<T>, dim3(S, 9), dim3(NT), 0, st, x, dy, y, g, dw_chunk(P, S), ws);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL(dw_combine_kernel<false>, dim3((9 * CH * CH + CH) / 16), dim3(NT), 0, st, ws, S, dw, db);
  DL4SS_CHECK_LAUNCH();
  if (dx) {
    const long long M0 = (long long)g.N * ((g.Hin + 1) >> 1) * ((g.Win + 1) >> 1);  // the (even, even) class
    hipLaunchKernelGGL((conv64_igemm_kernel<T, true>), dim3(cdiv(M0, BM), 4), dim3(NT), 0, st, dy, y, w,
                       (const float*)nullptr, g, dx);
    DL4SS_CHECK_LAUNCH();
  }
  return 0;
}

template <typename T>
int conv1_bwd_t(const float* x, const T* y, const T* dy, const float* w, Geom g, float* dx, float* dw, float* db,
                float* ws, hipStream_t st) {
  const long long P = (long long)g.N * g.Hout * g.Wout;
  const int S = dw_splits(P, C1_CHUNK, C1_MAX_SPLIT);
  hipLaunchKernelGGL(conv1_dw_part_kernel<T>, dim3(S), dim3(NT), 0, st, x, dy, y, g, (P + S - 1) / S, ws);
  DL4SS_CHECK_LAUNCH();
  hipLaunchKernelGGL(dw_combine_kernel<true>, dim3(CH * C1_ROWS / 16), dim3(NT), 0, st, ws, S, dw, db);
  DL4SS_CHECK_LAUNCH();
  if (dx) {
    const int tilesH = (int)cdiv((g.Hin + 1) >> 1, DX_TH), tilesW = (int)cdiv((g.Win + 1) >> 1, DX_TW);
    hipLaunchKernelGGL(conv1_dx_kernel<T>, dim3((unsigned)((long long)g.N * tilesH * tilesW)), dim3(NT), 0, st, dy, y,
                       w, g, tilesH, tilesW, dx);
    DL4SS_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

// Layer sizes of a (T, F) map: hw = {H1, W1, H2, W2, H3, W3}; returns the feature count 64 H3 W3 of
// final.weight, or -1 when the map is smaller than 15 x 15.  Host only.
DL4SS_API int dl4ss_disc_dims(int T, int F, int hw[6]) {
  if (T < 15 || F < 15) return -1;
  int h = T, w = F;
  for (int l = 0; l < 3; ++l) {
    h = out_dim(h);
    w = out_dim(w);
    if (hw) {
      hw[2 * l] = h;
      hw[2 * l + 1] = w;
    }
  }
  const long long feat = (long long)CH * h * w;
  return feat < (1LL << 31) ? (int)feat : -1;
}

// Bytes of the workspace the three *_bwd calls of N maps of (T, F) share (the largest layer's split-K
// partials), or -1 for an unsupported size.  Host only.
DL4SS_API long long dl4ss_disc_ws_bytes(int N, int T, int F) {
  int hw[6];
  if (N <= 0 || dl4ss_disc_dims(T, F, hw) < 0 || !geom_ok(N, T, F)) return -1;
  long long fl = conv1_ws_floats((long long)N * hw[0] * hw[1]);
  for (int l = 1; l < 3; ++l) {
    const long long f = conv64_ws_floats((long long)N * hw[2 * l] * hw[2 * l + 1]);
    fl = f > fl ? f : fl;
  }
  return fl * (long long)sizeof(float);
}

// x (N, T, F) fp32, w (64, 1, 3, 3), b (64) -> y1 (N, H1, W1, 64) fp32 (prec 0) or bf16 (prec 1)
DL4SS_API int dl4ss_disc_conv1_fwd(int prec, const float* x, const float* w, const float* b, int N, int T, int F,
                                   void* y1, void* stream) {
  DL4SS_REQUIRE(x && w && b && y1 && (prec == 0 || prec == 1) && geom_ok(N, T, F));
  const Geom g = make_geom(N, T, F);
  const unsigned nb = cdiv((long long)N * g.Hout * g.Wout, 16);
  if (prec == 0)
    hipLaunchKernelGGL(conv1_fwd_kernel<float>, dim3(nb), dim3(NT), 0, as_stream(stream), x, w, b, g, (float*)y1);
  else
    hipLaunchKernelGGL(conv1_fwd_kernel<bf16_t>, dim3(nb), dim3(NT), 0, as_stream(stream), x, w, b, g, (bf16_t*)y1);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// x (N, Hin, Win, 64), w (64, 64, 3, 3), b (64) -> y (N, Hout, Wout, 64) = relu(conv + b)
DL4SS_API int dl4ss_disc_conv64_fwd(int prec, const void* x, const float* w, const float* b, int N, int Hin, int Win,
                                    void* y, void* stream) {
  DL4SS_REQUIRE(x && w && b && y && (prec == 0 || prec == 1) && geom_ok(N, Hin, Win));
  const Geom g = make_geom(N, Hin, Win);
  const dim3 grid(cdiv((long long)N * g.Hout * g.Wout, BM));
  if (prec == 0)
    hipLaunchKernelGGL((conv64_igemm_kernel<float, false>), grid, dim3(NT), 0, as_stream(stream), (const float*)x,
                       (const float*)nullptr, w, b, g, (float*)y);
  else
    hipLaunchKernelGGL((conv64_igemm_kernel<bf16_t, false>), grid, dim3(NT), 0, as_stream(stream), (const bf16_t*)x,
                       (const bf16_t*)nullptr, w, b, g, (bf16_t*)y);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// y3 (N, H3, W3, 64), wf (64 H3 W3) in (c, h, w) order, bf (1) -> z (N), score (N) = sigmoid(z)
DL4SS_API int dl4ss_disc_head_fwd(int prec, const void* y3, const float* wf, const float* bf, int N, int H3, int W3,
                                  float* z, float* score, void* stream) {
  DL4SS_REQUIRE(y3 && wf && bf && z && score && (prec == 0 || prec == 1));
  DL4SS_REQUIRE(N > 0 && H3 > 0 && W3 > 0 && (long long)H3 * W3 * CH < (1LL << 31) / 2);
  if (prec == 0)
    hipLaunchKernelGGL(head_fwd_kernel<float>, dim3(N), dim3(NT), 0, as_stream(stream), (const float*)y3, wf, bf,
                       H3 * W3, z, score);
  else
    hipLaunchKernelGGL(head_fwd_kernel<bf16_t>, dim3(N), dim3(NT), 0, as_stream(stream), (const bf16_t*)y3, wf, bf,
                       H3 * W3, z, score);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// Backward of the head.  dscore (N) given: dz = dscore s (1 - s).  dscore NULL: the fused loss
// loss[0] = mean_n (score_n - target)^2 and its gradient.  Writes dz (N), dwf (64 H3 W3), dbf (1) and
// dy3 (N, H3, W3, 64) in the activation type; loss may be NULL.
DL4SS_API int dl4ss_disc_head_bwd(int prec, const void* y3, const float* wf, const float* score, const float* dscore,
                                  float target, int N, int H3, int W3, float* loss, float* dz, float* dwf, float* dbf,
                                  void* dy3, void* stream) {
  DL4SS_REQUIRE(y3 && wf && score && dz && dwf && dbf && dy3 && (prec == 0 || prec == 1));
  DL4SS_REQUIRE(N > 0 && H3 > 0 && W3 > 0 && (long long)H3 * W3 * CH < (1LL << 31) / 2);
  hipStream_t st = as_stream(stream);
  const int HW = H3 * W3;
  hipLaunchKernelGGL(head_dz_kernel, dim3(1), dim3(64), 0, st, score, dscore, target, N, loss, dz, dbf);
  DL4SS_CHECK_LAUNCH();
  if (prec == 0)
    hipLaunchKernelGGL(head_bwd_kernel<float>, dim3(cdiv((long long)HW * CH, NT)), dim3(NT), 0, st, (const float*)y3,
                       wf, dz, N, HW, dwf, (float*)dy3);
  else
    hipLaunchKernelGGL(head_bwd_kernel<bf16_t>, dim3(cdiv((long long)HW * CH, NT)), dim3(NT), 0, st,
                       (const bf16_t*)y3, wf, dz, N, HW, dwf, (bf16_t*)dy3);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// The adversarial step's loss heads: score (2 N) = [D(true maps); D(predicted maps)] -> loss (3) =
// {L_dt, L_df, L_adv} (means over the N maps, L_adv unweighted), dscore_dis (2 N) for the backward of
// L_dt + L_df over all maps, dscore_adv (N) = lambda dL_adv/dscore for the backward over the predicted maps
// (both go to dl4ss_disc_head_bwd as its dscore).
DL4SS_API int dl4ss_disc_adv_heads(const float* score, int N, float lambda, float* loss, float* dscore_dis,
                                   float* dscore_adv, void* stream) {
  DL4SS_REQUIRE(score && loss && dscore_dis && dscore_adv && N > 0);
  hipLaunchKernelGGL(adv_heads_kernel, dim3(1), dim3(64), 0, as_stream(stream), score, N, lambda, loss, dscore_dis,
                     dscore_adv);
  DL4SS_CHECK_LAUNCH();
  return 0;
}

// Backward of a 64 -> 64 layer from dy and the saved post-ReLU y (the gate y > 0 is applied on load).
// x (N, Hin, Win, 64) -> dw (64, 64, 3, 3), db (64) and, when dx is not NULL, dx (N, Hin, Win, 64) with
// every element written.  ws: dl4ss_disc_ws_bytes of the network the layer belongs to; checked against this
// layer's need.
DL4SS_API int dl4ss_disc_conv64_bwd(int prec, const void* x, const void* y, const void* dy, const float* w, int N,
                                    int Hin, int Win, void* dx, float* dw, float* db, void* ws, long long ws_bytes,
                                    void* stream) {
  DL4SS_REQUIRE(x && y && dy && w && dw && db && ws && (prec == 0 || prec == 1) && geom_ok(N, Hin, Win));
  const Geom g = make_geom(N, Hin, Win);
  DL4SS_REQUIRE(ws_bytes >= conv64_ws_floats((long long)N * g.Hout * g.Wout) * (long long)sizeof(float));
  if (prec == 0)
    return conv64_bwd_t<float>((const float*)x, (const float*)y, (const float*)dy, w, g, (float*)dx, dw, db,
                               (float*)ws, as_stream(stream));
  return conv64_bwd_t<bf16_t>((const bf16_t*)x, (const bf16_t*)y, (const bf16_t*)dy, w, g, (bf16_t*)dx, dw, db,
                              (float*)ws, as_stream(stream));
}

// Backward of conv1: x (N, T, F) fp32, y1 / dy1 (N, H1, W1, 64) -> dw (64, 1, 3, 3), db (64) and, when dx is
// not NULL, the input-map gradient dx (N, T, F) fp32 with every element written.
DL4SS_API int dl4ss_disc_conv1_bwd(int prec, const float* x, const void* y1, const void* dy1, const float* w, int N,
                                   int T, int F, float* dx, float* dw, float* db, void* ws, long long ws_bytes,
                                   void* stream) {
  DL4SS_REQUIRE(x && y1 && dy1 && w && dw && db && ws && (prec == 0 || prec == 1) && geom_ok(N, T, F));
  const Geom g = make_geom(N, T, F);
  DL4SS_REQUIRE(ws_bytes >= conv1_ws_floats((long long)N * g.Hout * g.Wout) * (long long)sizeof(float));
  if (prec == 0)
    return conv1_bwd_t<float>(x, (const float*)y1, (const float*)dy1, w, g, dx, dw, db, (float*)ws,
                              as_stream(stream));
  return conv1_bwd_t<bf16_t>(x, (const bf16_t*)y1, (const bf16_t*)dy1, w, g, dx, dw, db, (float*)ws,
                             as_stream(stream));
}
