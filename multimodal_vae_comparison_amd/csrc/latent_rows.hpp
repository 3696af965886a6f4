// The frame shared by the fused latent ops (latent.hip: product of experts; tcfusion.hip: total-correlation fusion;
// jsfusion.hip: Jensen-Shannon fusion; mixprior.hip: mixture-of-experts prior; mmplus.hip: MMVAE+'s split latents): one
// wavefront per sample, lanes over the latent dimension in POE_SLOTS column slots of 64.  Around each op's own arithmetic:
// the prior scale, the raw heads (lv = softmax(u) + 1e-6 applied by the kernels, both ways), the workgroup's partial
// prior-gradient row, the fold of these rows into dtheta, and the host side's support rule, workspace size and fold launch.
// The pointer tables come in as arrays of MMVAE_MAX_EXPERTS pointers: mmvae_tc_*_args, mmvae_poe_*_args and
// mmvae_mmplus_*_args all fit.  The arithmetic mixprior.hip and mmplus.hip share stands on this frame in mixture_rows.hpp.
#pragma once
#include "common.hpp"

// one wave per sample up to this many waves, then samples round robin (round 4: 128 -> 512; a wave's samples are a serial
// chain of L2 round trips: same box, ms/step of the cfg2 step at batch 512 / 1000 with 128 / 256 / 512 waves: 0.928 / 0.921 /
// 0.919 and 1.581 / 1.564 / 1.557)
#define POE_MAX_WAVES 512
#define POE_SLOTS 4  // D <= 64 * POE_SLOTS

// ---------------------------------------------------------------------------------------------
// prior sigma: softmax(theta) * D   (models/mmvae_models.py:274-276), computed per wave
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void prior_sigma(const float* __restrict__ theta, int D, int lane, float sp[POE_SLOTS],
                                            float sm[POE_SLOTS]) {
  float mx = -INFINITY;
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    int d = lane + 64 * s;
    if (d < D) mx = fmaxf(mx, theta[d]);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    int d = lane + 64 * s;
    sm[s] = d < D ? expf(theta[d] - mx) : 0.f;
    sum += sm[s];
  }
  sum = wave_sum(sum);
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    sm[s] = sm[s] / sum;
    sp[s] = sm[s] * (float)D;
  }
}

// statistics of softmax(u[0..D)) for one row: max and 1 / sum exp  (raw heads: lv = softmax(u) + 1e-6 computed here
// instead of by a head_softmax launch per tower and direction)
__device__ __forceinline__ void row_softmax_stats(const float* __restrict__ u, int D, int lane, float* mx_out,
                                                  float* inv_out) {
  float mx = -INFINITY;
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    const int d = lane + 64 * s;
    if (d < D) mx = fmaxf(mx, u[d]);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    const int d = lane + 64 * s;
    if (d < D) sum += expf(u[d] - mx);
  }
  sum = wave_sum(sum);
  *mx_out = mx;
  *inv_out = 1.0f / sum;
}

// raw heads: row_softmax_stats of every expert's row (`row` = the row's offset in the strided expert tensors)
__device__ __forceinline__ void raw_head_stats(const float* const lv[MMVAE_MAX_EXPERTS], int E, size_t row, int D, int lane,
                                               float umx[MMVAE_MAX_EXPERTS], float uinv[MMVAE_MAX_EXPERTS]) {
#pragma unroll
  for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e)
    if (e < E) row_softmax_stats(lv[e] + row, D, lane, &umx[e], &uinv[e]);
}

// raw heads, backward through lv = softmax(u) + 1e-6:  du = s (dlv - sum(s dlv)),  s = lv - 1e-6.  dlv[e] holds d/dlv of the
// row and receives d/du; udot[e]: this lane's share of sum(s dlv)
__device__ __forceinline__ void raw_head_bwd(const float* const lv[MMVAE_MAX_EXPERTS], float* const dlv[MMVAE_MAX_EXPERTS],
                                             int E, size_t row, int D, int lane,
                                             const float umx[MMVAE_MAX_EXPERTS], const float uinv[MMVAE_MAX_EXPERTS],
                                             const float udot[MMVAE_MAX_EXPERTS]) {
#pragma unroll
  for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
    if (e >= E) continue;
    const float dot = wave_sum(udot[e]);
#pragma unroll
    for (int s = 0; s < POE_SLOTS; ++s) {
      const int d = lane + 64 * s;
      if (d < D) {
        const size_t oi = row + d;
        const float sv = expf(lv[e][oi] - umx[e]) * uinv[e];
        // (D == 1: the softmax of one logit is the constant 1 and du is 0; s = lv - 1e-6 in `dot` is rounded, and
        // s (dlv - s dlv) came out as 6e-8 dlv)
        dlv[e][oi] = D == 1 ? 0.f : sv * (dlv[e][oi] - dot);
      }
    }
  }
}

__device__ __forceinline__ float kl_elem(float mu, float s, float sp) {
  float r = s / sp, m = mu / sp;
  float vr = r * r;
  return 0.5f * (vr + m * m - 1.0f - logf(vr));
}

static inline int poe_blocks(int B) {
  int waves = B < POE_MAX_WAVES ? B : POE_MAX_WAVES;
  return (waves + 3) / 4;
}

// the workgroup's partial prior-gradient row (d loss / d sp) into row blockIdx.x of ws: its four waves in wave order
__device__ __forceinline__ void prior_grad_row(const float dsp[POE_SLOTS], float (*part)[64 * POE_SLOTS],
                                               float* __restrict__ ws, int D, int lane) {
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) part[threadIdx.x >> 6][lane + 64 * s] = dsp[s];
  __syncthreads();
  if ((int)threadIdx.x < D)
    ws[(size_t)blockIdx.x * D + threadIdx.x] =
        part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// The fold of the prior gradient: dtheta_d (+)= D * s_d * (dsp_d - sum_k s_k dsp_k), dsp = sum over the partial rows in ws.
// 4 waves split the rows (wave w takes rows w, w + 4, ... in that order), 8 independent loads in flight per lane, the four
// sums are combined in wave order through LDS (D <= 256).
// COHERENT: the partial rows were written by other workgroups of the SAME launch with agent-scope write-through stores
// (latent.hip: poe_ws_store); read them with agent-scope loads that bypass the (per-XCD, non-coherent) L2
template <bool COHERENT = false>
__device__ __forceinline__ void poe_theta_body(const float* __restrict__ theta, const float* __restrict__ ws,
                                               float* __restrict__ dtheta, int nrows, int D, int accumulate,
                                               float (*part)[64 * POE_SLOTS]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto ld = [&](size_t i) -> float {
    return COHERENT ? __hip_atomic_load(ws + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ws[i];
  };
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    const int d = lane + 64 * s;
    float acc = 0.f;
    if (d < D) {
      int r = wave;
      for (; r + 28 < nrows; r += 32) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ld((size_t)(r + 4 * u) * D + d);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
      }
      for (; r < nrows; r += 4) acc += ld((size_t)r * D + d);
    }
    part[wave][d] = acc;
  }
  __syncthreads();
  if (wave != 0) return;
  float sp[POE_SLOTS], sm[POE_SLOTS], dsp[POE_SLOTS];
  prior_sigma(theta, D, lane, sp, sm);
  float dot = 0.f;
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    const int d = lane + 64 * s;
    dsp[s] = part[0][d] + part[1][d] + part[2][d] + part[3][d];
    dot += dsp[s] * sm[s];
  }
  dot = wave_sum(dot);
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    const int d = lane + 64 * s;
    if (d < D) {
      float g = (float)D * sm[s] * (dsp[s] - dot);
      dtheta[d] = accumulate ? dtheta[d] + g : g;
    }
  }
}

// the fold as a launch of its own behind tcfusion.hip's, jsfusion.hip's, mixprior.hip's and mmplus.hip's backward kernels,
// whose workgroups each leave one partial row in ws
static __global__ __launch_bounds__(256) void theta_fold_kernel(const float* __restrict__ theta, const float* __restrict__ ws,
                                                                float* __restrict__ dtheta, int nrows, int D,
                                                                int accumulate) {
  __shared__ float part[4][64 * POE_SLOTS];
  poe_theta_body<false>(theta, ws, dtheta, nrows, D, accumulate, part);
}

// ---- host side of the four ops with one partial row per workgroup ---------------------------------------------------
static inline bool fusion_supported(int E, int D) { return E <= MMVAE_MAX_EXPERTS && D <= 64 * POE_SLOTS; }

static inline size_t fusion_ws_floats(int B, int D) {
  if (B <= 0 || D <= 0 || D > 64 * POE_SLOTS) return 0;
  return (size_t)poe_blocks(B) * D;
}

// behind a backward kernel of poe_blocks(B) workgroups on the same stream; dtheta == NULL: the prior gradient is not wanted
static inline void launch_theta_fold(const float* theta, const float* ws, float* dtheta, int B, int D, int accumulate,
                                     mmvae_stream_t stream) {
  if (dtheta)
    hipLaunchKernelGGL(theta_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, theta, ws, dtheta, poe_blocks(B), D,
                       accumulate ? 1 : 0);
}
