// Row helpers shared by the fused latent ops (latent.hip: product of experts; tcfusion.hip: total-correlation fusion):
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

