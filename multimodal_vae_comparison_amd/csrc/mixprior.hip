// Mixture-of-experts prior (MMVM VAE: Sutter et al., "Unity by Diversity", NeurIPS 2024) for gfx950: one reparameterised
// sample from EVERY one of the E unimodal posteriors, the one-sample estimate of every posterior's KL to the uniform mixture
// of all E (the data-dependent prior), its closed-form KL to the fixed prior and the responsibilities, forward and backward,
// in one launch each way (+ the fold of the prior gradient).  The layout is jsfusion.hip's: one wavefront per sample, lanes
// over the latent dimension in POE_SLOTS column slots, wave-shuffle row sums; no atomics and no in-launch election -- every
// sum is taken in one fixed order.
//
// Expert j is q_j = N(mu_j, sigma_j = lv_j) (the head read as the SCALE, as MOE samples from it), the fixed prior is
// N(0, sp), sp = softmax(theta) D.  Per row, with z_m = mu_m + sigma_m eps_m and h = (1/E) sum_j q_j:
//   kl_mix[m] = log q_m(z_m) - log h(z_m),   resp[m][j] = q_j(z_m) / sum_k q_k(z_m)      (mixture_rows.hpp: the arithmetic,
//   kl_std[m] = sum_d KL(N(mu_m, sigma_m) || N(0, sp))                                     forward and backward)
// Backward, with g'_m = dkl[E + m], gz_m = dz[m], r = 1 / sp^2, the mixture's pair terms come on top of
//   dmu_m = gz_m + g'_m mu_m r,   dsg_m = gz_m eps_m + g'_m (sigma_m r - 1 / sigma_m);
//   dsp = sum_m g'_m (1 - (sigma_m^2 + mu_m^2) r) / sp.
#include "common.hpp"
#include "mixture_rows.hpp"

__global__ __launch_bounds__(256) void mixprior_fwd_kernel(mmvae_poe_fwd_args a, const float* __restrict__ theta,
                                                           float* __restrict__ kl, float* __restrict__ resp, int E, int B,
                                                           int D, int ld, int raw) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  float sp[POE_SLOTS], sm[POE_SLOTS];
  prior_sigma(theta, D, lane, sp, sm);
  const float logE = logf((float)E);
  for (int b = wave; b < B; b += nwaves) {
    float dl[MMVAE_MAX_EXPERTS][MMVAE_MAX_EXPERTS], ks[MMVAE_MAX_EXPERTS];
#pragma unroll
    for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {
      ks[m] = 0.f;
#pragma unroll
      for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j) dl[m][j] = 0.f;
    }
    float umx[MMVAE_MAX_EXPERTS], uinv[MMVAE_MAX_EXPERTS];
    if (raw) raw_head_stats(a.lv, E, (size_t)b * ld, D, lane, umx, uinv);
#pragma unroll
    for (int s = 0; s < POE_SLOTS; ++s) {
      const int d = lane + 64 * s;
      if (d < D) {
        const size_t o = (size_t)b * D + d;    // contiguous (B,D) tensors
        const size_t oi = (size_t)b * ld + d;  // strided expert tensors
        float mu[MMVAE_MAX_EXPERTS], sg[MMVAE_MAX_EXPERTS], ep[MMVAE_MAX_EXPERTS];
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          mu[e] = a.mu[e][oi];
          sg[e] = a.lv[e][oi];
          if (raw) sg[e] = raw_head_scale(sg[e], umx[e], uinv[e]);
          ep[e] = a.eps[e][o];
          a.z[e][o] = mu[e] + sg[e] * ep[e];
          ks[e] += kl_elem(mu[e], sg[e], sp[s]);
        }
#pragma unroll
        for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {
          if (m >= E) continue;
#pragma unroll
          for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j) {
            if (j >= E || j == m) continue;
            dl[m][j] += mix_dl(mu[m], sg[m], ep[m], mu[j], sg[j]);
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {
      if (m >= E) continue;
      const float kstd = wave_sum(ks[m]);
      mix_row_finish(dl, m, E, B, b, lane, logE, kl, resp);
      if (lane == 0) kl[(size_t)(E + m) * B + b] = kstd;
    }
  }
}

// a.dz[m] / dkl == NULL: that upstream gradient is absent and counts as zeros
__global__ __launch_bounds__(256) void mixprior_bwd_kernel(mmvae_poe_bwd_args a, const float* __restrict__ theta,
                                                           const float* __restrict__ resp, const float* __restrict__ dkl,
                                                           float* __restrict__ ws, int E, int B, int D, int ld, int raw) {
  __shared__ float part[4][64 * POE_SLOTS];
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  float sp[POE_SLOTS], sm[POE_SLOTS], dsp[POE_SLOTS];
  prior_sigma(theta, D, lane, sp, sm);
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) dsp[s] = 0.f;
  for (int b = wave; b < B; b += nwaves) {
    float c[MMVAE_MAX_EXPERTS][MMVAE_MAX_EXPERTS], gs[MMVAE_MAX_EXPERTS];
    mix_upstream(dkl, resp, E, B, b, c, gs);
    float umx[MMVAE_MAX_EXPERTS], uinv[MMVAE_MAX_EXPERTS], udot[MMVAE_MAX_EXPERTS];
#pragma unroll
    for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) udot[e] = 0.f;
    if (raw) raw_head_stats(a.lv, E, (size_t)b * ld, D, lane, umx, uinv);
#pragma unroll
    for (int s = 0; s < POE_SLOTS; ++s) {
      const int d = lane + 64 * s;
      if (d < D) {
        const size_t o = (size_t)b * D + d;    // contiguous (B,D) tensors
        const size_t oi = (size_t)b * ld + d;  // strided expert tensors
        float mu[MMVAE_MAX_EXPERTS], sg[MMVAE_MAX_EXPERTS], ep[MMVAE_MAX_EXPERTS], inv[MMVAE_MAX_EXPERTS];
        float dmu[MMVAE_MAX_EXPERTS], dsg[MMVAE_MAX_EXPERTS];
        const float r = 1.0f / (sp[s] * sp[s]);
        float dspv = 0.f;
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          mu[e] = a.mu[e][oi];
          sg[e] = a.lv[e][oi];
          if (raw) sg[e] = raw_head_scale(sg[e], umx[e], uinv[e]);
          ep[e] = a.eps[e][o];
          inv[e] = 1.0f / sg[e];
          const float gz = a.dz[e] ? a.dz[e][o] : 0.f;
          dmu[e] = gz + gs[e] * (mu[e] * r);
          dsg[e] = gz * ep[e] + gs[e] * (sg[e] * r - inv[e]);
          dspv += gs[e] * ((1.0f - (sg[e] * sg[e] + mu[e] * mu[e]) * r) / sp[s]);
        }
        dsp[s] += dspv;
#pragma unroll
        for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {      // sample m: its own expert's terms and every other expert's
          if (m >= E) continue;
#pragma unroll
          for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j) {
            if (j >= E || j == m) continue;
            mix_pair_bwd(mu[m], sg[m], ep[m], inv[m], mu[j], sg[j], inv[j], c[m][j], dmu[m], dsg[m], dmu[j], dsg[j]);
          }
        }
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          a.dmu[e][oi] = dmu[e];
          a.dlv[e][oi] = dsg[e];
          udot[e] += (sg[e] - 1e-6f) * dsg[e];
        }
      }
    }
    if (raw) raw_head_bwd(a.lv, a.dlv, E, (size_t)b * ld, D, lane, umx, uinv, udot);
  }
  prior_grad_row(dsp, part, ws, D, lane);
}

extern "C" size_t mmvae_mixprior_ws_floats(int B, int D) { return fusion_ws_floats(B, D); }

extern "C" int mmvae_mixprior_fwd(const mmvae_poe_fwd_args* a, const float* theta, float* kl, float* resp, int E, int B,
                                  int D, int ld_in, int raw_heads, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && theta && kl && resp && B > 0 && D > 0 && E > 0 && ld_in >= D);
  if (!fusion_supported(E, D)) return MMVAE_ERR_UNSUPPORTED;
  for (int e = 0; e < E; ++e) MMVAE_CHECK_ARG(a->mu[e] && a->lv[e] && a->eps[e] && a->z[e]);
  hipLaunchKernelGGL(mixprior_fwd_kernel, dim3(poe_blocks(B)), dim3(256), 0, (hipStream_t)stream, *a, theta, kl, resp, E,
                     B, D, ld_in, raw_heads ? 1 : 0);
  return mmvae_launch_status();
}

extern "C" int mmvae_mixprior_bwd(const mmvae_poe_bwd_args* a, const float* theta, const float* resp, const float* dkl,
                                  float* dtheta, float* ws, int E, int B, int D, int ld_in, int raw_heads, int accumulate,
                                  mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && theta && resp && ws && B > 0 && D > 0 && E > 0 && ld_in >= D);
  if (!fusion_supported(E, D)) return MMVAE_ERR_UNSUPPORTED;
  for (int e = 0; e < E; ++e) MMVAE_CHECK_ARG(a->mu[e] && a->lv[e] && a->eps[e] && a->dmu[e] && a->dlv[e]);
  hipLaunchKernelGGL(mixprior_bwd_kernel, dim3(poe_blocks(B)), dim3(256), 0, (hipStream_t)stream, *a, theta, resp, dkl, ws, E, B, D,
                     ld_in, raw_heads ? 1 : 0);
  launch_theta_fold(theta, ws, dtheta, B, D, accumulate, stream);
  return mmvae_launch_status();
}
