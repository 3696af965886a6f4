// The mixture-of-posteriors term of mixprior.hip (MMVM) and mmplus.hip (MMVAE+'s shared columns), on latent_rows.hpp's
// frame: every formula of it stands here once.  Expert j is q_j = N(mu_j, sigma_j), sample m is z_m = mu_m + sigma_m eps_m,
// h = (1/E) sum_j q_j.  Per element, for every ordered pair m != j:
//   u_mj = ((mu_m - mu_j) + sigma_m eps_m) / sigma_j                                       (z_m - mu_j) / sigma_j
//   D_mj = sum_d [ -1/2 (u_mj - eps_m)(u_mj + eps_m) - log(sigma_j / sigma_m) ]            log q_j(z_m) - log q_m(z_m), D_mm = 0
//   kl_mix[m] = log E - (max_j D_mj + log sum_j exp(D_mj - max_j D_mj)),   resp[m][j] = softmax_j D_mj
// backward, c_mj = -dkl[m] resp[m][j]:
//   dmu_m -= c_mj u_mj / sigma_j                             dmu_j += c_mj u_mj / sigma_j
//   dsg_m += c_mj (1 / sigma_m - u_mj eps_m / sigma_j)       dsg_j += c_mj (u_mj^2 - 1) / sigma_j
// Only differences of log-densities are formed -- at D = 256 the absolute ones reach the hundreds and their difference
// keeps their rounding, at scales of 1e-5 log sigma does (float32 on the host against float64: 4.8e-5 and 6.8e-5 of a KL
// entry against 2.7e-6 and 7.4e-7 in this form) --, and sample m is walked outermost: every sum has one fixed order.
// The pair functions take one element of one ordered pair: the walk over the columns and the two loops over (m, j) stay in
// each kernel.  With the loops inside a function (arrays by reference, by pointer, or a lambda over the pair) the compiler
// fuses 28 more multiply-add pairs per kernel and the results leave the text's by an ulp; this way they do not.  The whole
// sweep as one function template over a per-op source of eps, z and dz cost mixprior.hip a wave per SIMD both ways (191
// and 255 + 49 AGPRs against 160 and 254 VGPRs).
#pragma once
#include "latent_rows.hpp"

// raw heads: sigma = softmax(u) + 1e-6 of one element, from raw_head_stats' row statistics
__device__ __forceinline__ float raw_head_scale(float v, float umx, float uinv) { return expf(v - umx) * uinv + 1e-6f; }

// u_mj of one element: (z_m - mu_j) / sigma_j, formed from the difference of the means
__device__ __forceinline__ float mix_u(float mu_m, float sg_m, float ep_m, float mu_j, float sg_j) {
  return ((mu_m - mu_j) + sg_m * ep_m) / sg_j;
}

// one element's share of D_mj
__device__ __forceinline__ float mix_dl(float mu_m, float sg_m, float ep_m, float mu_j, float sg_j) {
  const float u = mix_u(mu_m, sg_m, ep_m, mu_j, sg_j);
  return -0.5f * (u - ep_m) * (u + ep_m) - logf(sg_j / sg_m);
}

// sample m's row: the wave sums of dl[m][*] (left in place), then lane 0 writes kl row m and resp[m][*] of sample b
__device__ __forceinline__ void mix_row_finish(float (&dl)[MMVAE_MAX_EXPERTS][MMVAE_MAX_EXPERTS], int m, int E, int B, int b,
                                               int lane, float logE, float* __restrict__ kl, float* __restrict__ resp) {
  float mx = 0.f;      // D_mm = 0 is one of the E
#pragma unroll
  for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j) {
    if (j >= E || j == m) continue;
    dl[m][j] = wave_sum(dl[m][j]);
    mx = fmaxf(mx, dl[m][j]);
  }
  float ex[MMVAE_MAX_EXPERTS], S = 0.f;
#pragma unroll
  for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j) {
    if (j >= E) continue;
    ex[j] = expf(dl[m][j] - mx);      // (dl[m][m] is the 0 it was set to)
    S += ex[j];
  }
  if (lane == 0) {
    kl[(size_t)m * B + b] = logE - (mx + logf(S));
    const float invS = 1.0f / S;
#pragma unroll
    for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j)
      if (j < E) resp[((size_t)m * E + j) * B + b] = ex[j] * invS;
  }
}

// sample b's upstream gradients: c[m][j] = -dkl[m] resp[m][j] (m != j), gs[m] = dkl[E + m]; dkl == NULL: zeros
__device__ __forceinline__ void mix_upstream(const float* __restrict__ dkl, const float* __restrict__ resp, int E, int B, int b,
                                             float (&c)[MMVAE_MAX_EXPERTS][MMVAE_MAX_EXPERTS], float (&gs)[MMVAE_MAX_EXPERTS]) {
#pragma unroll
  for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {
    if (m >= E) continue;
    const float g = dkl ? dkl[(size_t)m * B + b] : 0.f;
    gs[m] = dkl ? dkl[(size_t)(E + m) * B + b] : 0.f;
#pragma unroll
    for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j)
      if (j < E && j != m) c[m][j] = -g * resp[((size_t)m * E + j) * B + b];
  }
}

// one element's terms of the ordered pair (m, j), c = c[m][j], inv = 1 / sg: onto sample m's own expert and onto expert j
__device__ __forceinline__ void mix_pair_bwd(float mu_m, float sg_m, float ep_m, float inv_m, float mu_j, float sg_j, float inv_j,
                                             float c, float& dmu_m, float& dsg_m, float& dmu_j, float& dsg_j) {
  const float u = mix_u(mu_m, sg_m, ep_m, mu_j, sg_j);
  const float t = c * (u * inv_j);
  dmu_m -= t;
  dmu_j += t;
  dsg_m += c * (inv_m - u * ep_m * inv_j);
  dsg_j += c * ((u * u - 1.0f) * inv_j);
}
