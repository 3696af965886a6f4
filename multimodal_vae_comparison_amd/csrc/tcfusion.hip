// Total-correlation fusion (MVTCAE) for gfx950: product of experts -> one reparameterised sample -> KL of the joint to the
// prior and to EVERY expert, forward and backward, in one launch each way (+ the fold of the prior gradient).
// The layout is latent.hip's: one wavefront per sample, lanes over the latent dimension in POE_SLOTS column slots,
// wave-shuffle row sums; no atomics and no in-launch election -- every sum is taken in one fixed order.
//
// Per element (fixed b, d), a_e = exp(lv_e) + 1e-8, T_e = 1 / a_e, P = sum T_e, muJ = sum mu_e T_e / P, V = 1 / P:
//   z    = muJ + V eps
//   kl_E = 1/2 ((V / sp)^2 + (muJ / sp)^2 - 1 - log (V / sp)^2)                       joint || N(0, sp)
//   kl_e = -log(T_e V) + 1/2 T_e^2 (V^2 + (muJ - mu_e)^2) - 1/2                        joint || N(mu_e, sigma = a_e)
// Backward, with gz = dz, gP = dkl[E], g_e = dkl[e], m_e = muJ - mu_e:
//   G_mu  = gz     + gP muJ / sp^2         + sum_e g_e T_e^2 m_e
//   G_var = gz eps + gP (V / sp^2 - P)     + sum_e g_e (T_e^2 V - P)
//   dmu_e = G_mu T_e V - g_e T_e^2 m_e
//   dT_e  = -G_mu m_e V - G_var V^2 + g_e (T_e (V^2 + m_e^2) - a_e)
//   dlv_e = dT_e (-exp(lv_e) T_e^2)
//   dsp  += gP (1 - (V^2 + muJ^2) / sp^2) / sp
#include "common.hpp"
#include "latent_rows.hpp"

__global__ __launch_bounds__(256) void tc_fwd_kernel(mmvae_tc_fwd_args a, const float* __restrict__ theta,
                                                     const float* __restrict__ eps, float* __restrict__ joint,
                                                     float* __restrict__ kl, float* __restrict__ z, int E, int B, int D,
                                                     int ld, int raw) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  float sp[POE_SLOTS], sm[POE_SLOTS];
  prior_sigma(theta, D, lane, sp, sm);
  for (int b = wave; b < B; b += nwaves) {
    float klacc[MMVAE_MAX_EXPERTS], klp = 0.f;
#pragma unroll
    for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) klacc[e] = 0.f;
    float umx[MMVAE_MAX_EXPERTS], uinv[MMVAE_MAX_EXPERTS];
    if (raw) raw_head_stats(a.lv, E, (size_t)b * ld, D, lane, umx, uinv);
#pragma unroll
    for (int s = 0; s < POE_SLOTS; ++s) {
      const int d = lane + 64 * s;
      if (d < D) {
        const size_t o = (size_t)b * D + d;    // contiguous (B,D) tensors
        const size_t oi = (size_t)b * ld + d;  // strided expert tensors
        float mu[MMVAE_MAX_EXPERTS], T[MMVAE_MAX_EXPERTS];
        float P = 0.f, S = 0.f;
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          mu[e] = a.mu[e][oi];
          float lv = a.lv[e][oi];
          if (raw) lv = expf(lv - umx[e]) * uinv[e] + 1e-6f;
          T[e] = 1.0f / (expf(lv) + 1e-8f);
          P += T[e];
          S += mu[e] * T[e];
        }
        const float muJ = S / P, varJ = 1.0f / P;
        joint[o] = muJ;
        joint[(size_t)B * D + o] = varJ;
        z[o] = muJ + varJ * eps[o];
        klp += kl_elem(muJ, varJ, sp[s]);
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          const float m = muJ - mu[e];
          klacc[e] += -logf(T[e] * varJ) + 0.5f * T[e] * T[e] * (varJ * varJ + m * m) - 0.5f;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
      if (e >= E) continue;
      const float v = wave_sum(klacc[e]);
      if (lane == 0) kl[(size_t)e * B + b] = v;
    }
    klp = wave_sum(klp);
    if (lane == 0) kl[(size_t)E * B + b] = klp;
  }
}

// dz / dkl == NULL: that upstream gradient is absent and counts as zeros
__global__ __launch_bounds__(256) void tc_bwd_kernel(mmvae_tc_bwd_args a, const float* __restrict__ theta,
                                                     const float* __restrict__ eps, const float* __restrict__ dz,
                                                     const float* __restrict__ dkl, float* __restrict__ ws, int E, int B,
                                                     int D, int ld, int raw) {
  __shared__ float part[4][64 * POE_SLOTS];
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  float sp[POE_SLOTS], sm[POE_SLOTS], dsp[POE_SLOTS];
  prior_sigma(theta, D, lane, sp, sm);
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) dsp[s] = 0.f;
  for (int b = wave; b < B; b += nwaves) {
    float gk[MMVAE_MAX_EXPERTS];
#pragma unroll
    for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) gk[e] = (e < E && dkl) ? dkl[(size_t)e * B + b] : 0.f;
    const float gP = dkl ? dkl[(size_t)E * B + b] : 0.f;
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
        const float isp2 = 1.0f / (sp[s] * sp[s]);
        float mu[MMVAE_MAX_EXPERTS], lv[MMVAE_MAX_EXPERTS], ex[MMVAE_MAX_EXPERTS], T[MMVAE_MAX_EXPERTS];
        float P = 0.f, S = 0.f;
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          mu[e] = a.mu[e][oi];
          lv[e] = a.lv[e][oi];
          if (raw) lv[e] = expf(lv[e] - umx[e]) * uinv[e] + 1e-6f;
          ex[e] = expf(lv[e]);
          T[e] = 1.0f / (ex[e] + 1e-8f);
          P += T[e];
          S += mu[e] * T[e];
        }
        const float muJ = S / P, varJ = 1.0f / P;
        const float gz = dz ? dz[o] : 0.f;
        float Gmu = gz + gP * muJ * isp2;
        float Gvar = gz * eps[o] + gP * (varJ * isp2 - P);
        dsp[s] += gP * (1.0f - (varJ * varJ + muJ * muJ) * isp2) / sp[s];
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          const float t2 = T[e] * T[e];
          Gmu += gk[e] * t2 * (muJ - mu[e]);
          Gvar += gk[e] * (t2 * varJ - P);
        }
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          const float m = muJ - mu[e], t2 = T[e] * T[e];
          const float dmu = Gmu * T[e] * varJ - gk[e] * t2 * m;
          const float dT = -Gmu * m * varJ - Gvar * varJ * varJ +
                           gk[e] * (T[e] * (varJ * varJ + m * m) - (ex[e] + 1e-8f));
          const float dlv = dT * (-ex[e] * t2);
          a.dmu[e][oi] = dmu;
          a.dlv[e][oi] = dlv;
          udot[e] += (lv[e] - 1e-6f) * dlv;
        }
      }
    }
    if (raw) raw_head_bwd(a.lv, a.dlv, E, (size_t)b * ld, D, lane, umx, uinv, udot);
  }
  prior_grad_row(dsp, part, ws, D, lane);
}

extern "C" size_t mmvae_tc_fusion_ws_floats(int B, int D) { return fusion_ws_floats(B, D); }

extern "C" int mmvae_tc_fusion_fwd(const mmvae_tc_fwd_args* a, const float* theta, const float* eps, float* joint,
                                   float* kl, float* z, int E, int B, int D, int ld_in, int raw_heads,
                                   mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && theta && eps && joint && kl && z && B > 0 && D > 0 && E > 0 && ld_in >= D);
  if (!fusion_supported(E, D)) return MMVAE_ERR_UNSUPPORTED;
  for (int e = 0; e < E; ++e) MMVAE_CHECK_ARG(a->mu[e] && a->lv[e]);
  hipLaunchKernelGGL(tc_fwd_kernel, dim3(poe_blocks(B)), dim3(256), 0, (hipStream_t)stream, *a, theta, eps, joint, kl, z,
                     E, B, D, ld_in, raw_heads ? 1 : 0);
  return mmvae_launch_status();
}

extern "C" int mmvae_tc_fusion_bwd(const mmvae_tc_bwd_args* a, const float* theta, const float* eps, const float* dz,
                                   const float* dkl, float* dtheta, float* ws, int E, int B, int D, int ld_in,
                                   int raw_heads, int accumulate, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && theta && eps && ws && B > 0 && D > 0 && E > 0 && ld_in >= D);
  if (!fusion_supported(E, D)) return MMVAE_ERR_UNSUPPORTED;
  for (int e = 0; e < E; ++e) MMVAE_CHECK_ARG(a->mu[e] && a->lv[e] && a->dmu[e] && a->dlv[e]);
  hipLaunchKernelGGL(tc_bwd_kernel, dim3(poe_blocks(B)), dim3(256), 0, (hipStream_t)stream, *a, theta, eps, dz, dkl, ws, E, B, D,
                     ld_in, raw_heads ? 1 : 0);
  launch_theta_fold(theta, ws, dtheta, B, D, accumulate, stream);
  return mmvae_launch_status();
}
