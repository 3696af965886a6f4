// Generation coherence (TorchMMVAE.cross_coherence / joint_coherence): the two scoring kernels, forward only.
//   mmvae_text_decode_score: argmax over the alphabet of every decoded step (the first maximum) and, against target ids,
//     the number of matching letters over the shorter of the two strings.  One wave per sequence.
//   mmvae_cls_head: the head of A attribute classifiers in one launch -- relu(feats) W1^T + b1, relu, W2^T + b2, argmax,
//     comparison with the labels.  Plain fp32 FMA accumulation (the argmax decisions are the product); the hidden
//     256-vector lives in registers only.
#include <limits.h>

#include "common.hpp"

// ---- text ------------------------------------------------------------------------------------------------------------
#define TDS_WAVES 4

__global__ __launch_bounds__(TDS_WAVES * 64) void text_decode_score_kernel(const float* __restrict__ logits,
                                                                           const int* __restrict__ target_ids,
                                                                           const int* __restrict__ lengths,
                                                                           int* __restrict__ pred, int* __restrict__ letters,
                                                                           int N, int T, int V) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * TDS_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;      // (wave-uniform; no barrier below)
  const float* __restrict__ seq = logits + (size_t)n * T * V;
  const int len = target_ids ? min(max(lengths[n], 0), T) : 0;
  int same = 0;
  for (int t = 0; t < T; ++t) {
    const float* __restrict__ row = seq + (size_t)t * V;
    // the lane's candidates come in rising index order: a strict comparison keeps its first maximum
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int v = lane; v < V; v += 64) {
      const float x = row[v];
      if (x > bv || bi == INT_MAX) {
        bv = x;
        bi = v;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) {      // equal maxima: the first index wins
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) pred[(size_t)n * T + t] = bi;
    if (t < len && bi == target_ids[(size_t)n * T + t]) same += 1;
  }
  if (target_ids && lane == 0) letters[n] = same;
}

extern "C" int mmvae_text_decode_score(const float* logits, const int* target_ids, const int* lengths, int* pred,
                                       int* letters, int N, int T, int V, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(logits && pred && N > 0 && (!target_ids || (lengths && letters)));
  if (T < 1 || T > MMVAE_COH_MAX_STEPS || V < 2 || V > MMVAE_COH_MAX_VOCAB) return MMVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(text_decode_score_kernel, dim3((N + TDS_WAVES - 1) / TDS_WAVES), dim3(TDS_WAVES * 64), 0,
                     (hipStream_t)stream, logits, target_ids, lengths, pred, letters, N, T, V);
  return mmvae_launch_status();
}

// ---- classifier head -------------------------------------------------------------------------------------------------
#define CH_THREADS 256
#define CH_TR 32        // rows of a tile: 16 thread rows x 2
#define CH_KC 32        // columns of feats staged per pass
#define CH_IN MMVAE_COH_FEATS
#define CH_HID MMVAE_COH_HIDDEN

struct ClsClasses {
  int C[MMVAE_COH_MAX_CLASSIFIERS];
};

// grid (row tiles, classifiers).  Thread (ty, tx) = (tid / 16, tid % 16) owns rows 2 ty, 2 ty + 1 of the tile and the
// hidden units tx + 16 j, j < 16.  A pass stages relu(feats) (CH_TR x CH_KC) and W1 (256 x CH_KC) in LDS, both
// k-major, while the next pass's global loads are already in flight in registers.  The second layer is summed over the
// thread's 16 hidden units, then over the 16 threads of a row group by a fixed butterfly: the result does not depend on
// the launch shape or on what runs beside it.
__global__ __launch_bounds__(CH_THREADS) void cls_head_kernel(ClsClasses ncls, const float* __restrict__ feats,
                                                              const float* __restrict__ W1, const float* __restrict__ b1,
                                                              const float* __restrict__ W2, const float* __restrict__ b2,
                                                              const int* __restrict__ labels, int* __restrict__ pred,
                                                              float* __restrict__ logits, unsigned char* __restrict__ correct,
                                                              int* __restrict__ n_correct, int N, int Cmax) {
  __shared__ float Xs[CH_KC * CH_TR];
  __shared__ float Ws[CH_KC * CH_HID];
  const int a = blockIdx.y, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int C = ncls.C[a];
  const int row0 = blockIdx.x * CH_TR;
  const float* __restrict__ xa = feats + (size_t)a * N * CH_IN;
  const float* __restrict__ w1a = W1 + (size_t)a * CH_HID * CH_IN + (size_t)tid * CH_IN;      // hidden unit tid's row
  // staging role: feats row xr, columns xk .. xk + 3 of the pass; W1 row tid, all CH_KC columns of the pass
  const int xr = tid >> 3, xk = (tid & 7) * 4;
  const bool x_in = row0 + xr < N;
  const float* __restrict__ xsrc = xa + (size_t)(x_in ? row0 + xr : 0) * CH_IN + xk;

  f32x4 px, pw[CH_KC / 4];
  auto fetch = [&](int k0) {
    px = x_in ? *reinterpret_cast<const f32x4*>(xsrc + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < CH_KC / 4; ++q) pw[q] = *reinterpret_cast<const f32x4*>(w1a + k0 + 4 * q);
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) Xs[(xk + i) * CH_TR + xr] = fmaxf(px[i], 0.0f);
#pragma unroll
    for (int q = 0; q < CH_KC / 4; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) Ws[(4 * q + i) * CH_HID + tid] = pw[q][i];
  };

  float acc[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

  fetch(0);
  for (int k0 = 0; k0 < CH_IN; k0 += CH_KC) {
    stage();
    __syncthreads();
    if (k0 + CH_KC < CH_IN) fetch(k0 + CH_KC);
#pragma unroll 8
    for (int k = 0; k < CH_KC; ++k) {
      const float x0 = Xs[k * CH_TR + 2 * ty], x1 = Xs[k * CH_TR + 2 * ty + 1];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float w = Ws[k * CH_HID + tx + 16 * j];
        acc[0][j] = fmaf(x0, w, acc[0][j]);
        acc[1][j] = fmaf(x1, w, acc[1][j]);
      }
    }
    __syncthreads();
  }

  // hidden = relu(acc + b1); partial logits over the thread's 16 hidden units
  float part[2][MMVAE_COH_MAX_CLASSES];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int c = 0; c < MMVAE_COH_MAX_CLASSES; ++c) part[i][c] = 0.f;
  const float* __restrict__ b1a = b1 + (size_t)a * CH_HID;
  const float* __restrict__ w2a = W2 + (size_t)a * Cmax * CH_HID;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int u = tx + 16 * j;
    const float bb = b1a[u];
    const float h0 = fmaxf(acc[0][j] + bb, 0.0f), h1 = fmaxf(acc[1][j] + bb, 0.0f);
#pragma unroll
    for (int c = 0; c < MMVAE_COH_MAX_CLASSES; ++c)
      if (c < C) {
        const float w = w2a[c * CH_HID + u];
        part[0][c] = fmaf(h0, w, part[0][c]);
        part[1][c] = fmaf(h1, w, part[1][c]);
      }
  }
  // the 16 threads of a row group are 16 consecutive lanes of one wave
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int c = 0; c < MMVAE_COH_MAX_CLASSES; ++c)
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) part[i][c] += __shfl_xor(part[i][c], o, 64);

  if (tx < 2) {      // thread tx of the group finishes row 2 ty + tx
    const int n = row0 + 2 * ty + tx;
    if (n < N) {
      const float* __restrict__ b2a = b2 + (size_t)a * Cmax;
      float best = -INFINITY;
      int arg = 0;
#pragma unroll
      for (int c = 0; c < MMVAE_COH_MAX_CLASSES; ++c)
        if (c < C) {
          const float v = (tx == 0 ? part[0][c] : part[1][c]) + b2a[c];
          if (logits) logits[((size_t)a * N + n) * Cmax + c] = v;
          if (v > best) {      // strict: the first maximum wins
            best = v;
            arg = c;
          }
        }
      if (logits)
        for (int c = C; c < Cmax; ++c) logits[((size_t)a * N + n) * Cmax + c] = 0.f;
      pred[(size_t)a * N + n] = arg;
      if (labels) {
        const int y = labels[(size_t)a * N + n];
        const bool ok = y >= 0 && arg == y;
        correct[(size_t)a * N + n] = ok ? 1 : 0;
        if (ok) atomicAdd(n_correct + n, 1);      // (integers: the order of the classifiers does not show)
      }
    }
  }
}

extern "C" int mmvae_cls_head(const float* feats, const float* W1, const float* b1, const float* W2, const float* b2,
                              const int* n_classes, const int* labels, int* pred, float* logits, unsigned char* correct,
                              int* n_correct, int A, int N, int Cmax, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(feats && W1 && b1 && W2 && b2 && n_classes && pred && A > 0 && N > 0 && (!labels || (correct && n_correct)));
  if (A > MMVAE_COH_MAX_CLASSIFIERS || Cmax < 2 || Cmax > MMVAE_COH_MAX_CLASSES) return MMVAE_ERR_UNSUPPORTED;
  ClsClasses t;
  for (int a = 0; a < A; ++a) {
    if (n_classes[a] < 2 || n_classes[a] > Cmax) return MMVAE_ERR_UNSUPPORTED;
    t.C[a] = n_classes[a];
  }
  if (labels && hipMemsetAsync(n_correct, 0, (size_t)N * sizeof(int), (hipStream_t)stream) != hipSuccess)
    return MMVAE_ERR_LAUNCH;
  hipLaunchKernelGGL(cls_head_kernel, dim3((N + CH_TR - 1) / CH_TR, A), dim3(CH_THREADS), 0, (hipStream_t)stream, t, feats,
                     W1, b1, W2, b2, labels, pred, logits, correct, n_correct, N, Cmax);
  return mmvae_launch_status();
}
