// Row helpers shared by the fused latent ops (latent.hip: product of experts; tcfusion.hip: total-correlation fusion;
// jsfusion.hip: Jensen-Shannon fusion):
// one wavefront per sample, lanes over the latent dimension in POE_SLOTS column slots of 64.
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

__device__ __forceinline__ float kl_elem(float mu, float s, float sp) {
  float r = s / sp, m = mu / sp;
  float vr = r * r;
  return 0.5f * (vr + m * m - 1.0f - logf(vr));
}

static inline int poe_blocks(int B) {
  int waves = B < POE_MAX_WAVES ? B : POE_MAX_WAVES;
  return (waves + 3) / 4;
}

// The fold of the prior gradient behind tcfusion.hip's and jsfusion.hip's backward kernels, whose workgroups each leave one
// partial row of d loss / d sp in ws.
// dtheta_d (+)= D s_d (dsp_d - sum_k s_k dsp_k), dsp = the workgroups' partial rows summed in row order: wave w takes rows
// w, w + 4, ..., the four sums are combined in wave order (D <= 256)
static __global__ __launch_bounds__(256) void theta_fold_kernel(const float* __restrict__ theta, const float* __restrict__ ws,
                                                                float* __restrict__ dtheta, int nrows, int D,
                                                                int accumulate) {
  __shared__ float part[4][64 * POE_SLOTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) {
    const int d = lane + 64 * s;
    float acc = 0.f;
    if (d < D)
      for (int r = wave; r < nrows; r += 4) acc += ws[(size_t)r * D + d];
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
      const float g = (float)D * sm[s] * (dsp[s] - dot);
      dtheta[d] = accumulate ? dtheta[d] + g : g;
    }
  }
}

