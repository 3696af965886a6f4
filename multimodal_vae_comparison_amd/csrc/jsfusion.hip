// Jensen-Shannon fusion (mmJSD) for gfx950: the weighted geometric mean of the E unimodal posteriors and the prior (the
// "dynamic prior") -> the KL of every one of the E + 1 to it -> one reparameterised sample per row from the expert `sel`
// names, forward and backward, in one launch each way (+ the fold of the prior gradient).  The layout is tcfusion.hip's:
// one wavefront per sample, lanes over the latent dimension in POE_SLOTS column slots, wave-shuffle row sums; no atomics
// and no in-launch election -- every sum is taken in one fixed order.
//
// Expert j < E is N(mu_j, sigma_j = lv_j) (the head read as the SCALE, as MOE samples from it), j = E is the prior
// N(0, sp), sp = softmax(theta) D.  Per element (fixed b, d), with the weights pi_0 .. pi_E:
//   T_j = pi_j / sigma_j^2,  P = sum_j T_j,  f = sum_j T_j mu_j / P            dynamic prior N(f, P^-1/2)
//   m_j = mu_j - f = sum_i T_i (mu_j - mu_i) / P                               (the pairwise form: see below)
//   kl_j = 1/2 (-log(sigma_j^2 P) + P (sigma_j^2 + m_j^2) - 1)                 N(mu_j, sigma_j) || N(f, P^-1/2)
//   z    = mu_s + sigma_s eps,  s = sel[b]                                     (no expert has that index: z = 0)
// Backward, with g_j = dkl[j], gz = dz, [s] = 1 for the selected expert:
//   G_f   = -P sum_j g_j m_j,   G_P = 1/2 sum_j g_j (sigma_j^2 + m_j^2 - 1 / P)
//   dmu_i = g_i P m_i + G_f T_i / P + [s] gz
//   dT_i  = G_f m_i / P + G_P
//   dsg_i = g_i (P sigma_i - 1 / sigma_i) - 2 T_i dT_i / sigma_i + [s] gz eps
//   dsp   = dsg_E
// m_j is formed from the pairwise differences: sigma reaches 1e-6, P 1e12, and when one expert dominates mu_j - f
// cancels to float32 rounding before P multiplies its square.  log(sigma_j^2 P) is taken of the product, which lies in
// [pi_j, 1e13]: 2 log sigma_j + log P would add logarithms of up to -28 and +30 and keep their rounding (measured in
// float32 on the host over the tests' cases: 3.7e-6 of a KL entry against 1.0e-6).  The selected expert is found by
// comparing the loop index with sel[b] inside the unrolled loop, never by indexing the pointer table with it.
#include "common.hpp"
#include "latent_rows.hpp"

struct js_weights {
  float pi[MMVAE_MAX_EXPERTS];
  float prior;
};

// m_j of every expert and of the prior (mp) from the pairwise differences, summed in expert order, the prior's term last
__device__ __forceinline__ void js_centre(const float mu[MMVAE_MAX_EXPERTS], const float T[MMVAE_MAX_EXPERTS], float Tp,
                                          float invP, int E, float m[MMVAE_MAX_EXPERTS], float* mp) {
  float sp_acc = 0.f;
#pragma unroll
  for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j) {
    if (j >= E) continue;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < MMVAE_MAX_EXPERTS; ++i) {
      if (i >= E) continue;
      acc += T[i] * (mu[j] - mu[i]);
    }
    acc += Tp * mu[j];
    m[j] = acc * invP;
    sp_acc += T[j] * (0.f - mu[j]);
  }
  *mp = sp_acc * invP;
}

__global__ __launch_bounds__(256) void js_fwd_kernel(mmvae_tc_fwd_args a, js_weights w, const float* __restrict__ theta,
                                                     const float* __restrict__ eps, const int* __restrict__ sel,
                                                     float* __restrict__ prior, float* __restrict__ kl,
                                                     float* __restrict__ z, int E, int B, int D, int ld, int raw) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  float sp[POE_SLOTS], sm[POE_SLOTS];
  prior_sigma(theta, D, lane, sp, sm);
  for (int b = wave; b < B; b += nwaves) {
    const int sb = sel[b];
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
        float mu[MMVAE_MAX_EXPERTS], sg[MMVAE_MAX_EXPERTS], T[MMVAE_MAX_EXPERTS], m[MMVAE_MAX_EXPERTS];
        float P = 0.f, S = 0.f, zv = 0.f;
        const float ev = eps[o];
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          mu[e] = a.mu[e][oi];
          sg[e] = a.lv[e][oi];
          if (raw) sg[e] = expf(sg[e] - umx[e]) * uinv[e] + 1e-6f;
          T[e] = w.pi[e] / (sg[e] * sg[e]);
          P += T[e];
          S += mu[e] * T[e];
          if (e == sb) zv = mu[e] + sg[e] * ev;
        }
        const float Tp = w.prior / (sp[s] * sp[s]);
        P += Tp;
        const float invP = 1.0f / P;
        float mp;
        js_centre(mu, T, Tp, invP, E, m, &mp);
        prior[o] = S * invP;
        prior[(size_t)B * D + o] = 1.0f / sqrtf(P);
        z[o] = zv;
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          const float v = sg[e] * sg[e];
          klacc[e] += 0.5f * (-logf(v * P) + P * (v + m[e] * m[e]) - 1.0f);
        }
        klp += 0.5f * (-logf(sp[s] * sp[s] * P) + P * (sp[s] * sp[s] + mp * mp) - 1.0f);
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
__global__ __launch_bounds__(256) void js_bwd_kernel(mmvae_tc_bwd_args a, js_weights w, const float* __restrict__ theta,
                                                     const float* __restrict__ eps, const int* __restrict__ sel,
                                                     const float* __restrict__ dz, const float* __restrict__ dkl,
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
    const int sb = sel[b];
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
        float mu[MMVAE_MAX_EXPERTS], sg[MMVAE_MAX_EXPERTS], T[MMVAE_MAX_EXPERTS], m[MMVAE_MAX_EXPERTS];
        float P = 0.f;
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          mu[e] = a.mu[e][oi];
          sg[e] = a.lv[e][oi];
          if (raw) sg[e] = expf(sg[e] - umx[e]) * uinv[e] + 1e-6f;
          T[e] = w.pi[e] / (sg[e] * sg[e]);
          P += T[e];
        }
        const float Tp = w.prior / (sp[s] * sp[s]);
        P += Tp;
        const float invP = 1.0f / P;
        float mp;
        js_centre(mu, T, Tp, invP, E, m, &mp);
        const float gz = dz ? dz[o] : 0.f;
        const float gze = gz * eps[o];
        float sgm = 0.f, sgp = 0.f;      // sum_j g_j m_j, sum_j g_j (sigma_j^2 + m_j^2 - 1 / P): experts in order, then the prior
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          sgm += gk[e] * m[e];
          sgp += gk[e] * (sg[e] * sg[e] + m[e] * m[e] - invP);
        }
        sgm += gP * mp;
        sgp += gP * (sp[s] * sp[s] + mp * mp - invP);
        const float Gf = -P * sgm, GP = 0.5f * sgp;
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          const float dT = Gf * m[e] * invP + GP;
          float dmu = gk[e] * P * m[e] + Gf * T[e] * invP;
          float dsg = gk[e] * (P * sg[e] - 1.0f / sg[e]) - 2.0f * T[e] * dT / sg[e];
          if (e == sb) {
            dmu += gz;
            dsg += gze;
          }
          a.dmu[e][oi] = dmu;
          a.dlv[e][oi] = dsg;
          udot[e] += (sg[e] - 1e-6f) * dsg;
        }
        const float dTp = Gf * mp * invP + GP;
        dsp[s] += gP * (P * sp[s] - 1.0f / sp[s]) - 2.0f * Tp * dTp / sp[s];
      }
    }
    if (raw) raw_head_bwd(a.lv, a.dlv, E, (size_t)b * ld, D, lane, umx, uinv, udot);
  }
  prior_grad_row(dsp, part, ws, D, lane);
}

// pi_0 .. pi_E from the host: every one finite and >= 0, their sum > 0
static inline bool js_take_weights(const float* weights, int E, js_weights* w) {
  float sum = 0.f;
  for (int e = 0; e <= E; ++e) {
    if (!(weights[e] >= 0.f) || !std::isfinite(weights[e])) return false;
    sum += weights[e];
  }
  if (!(sum > 0.f) || !std::isfinite(sum)) return false;
  for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) w->pi[e] = e < E ? weights[e] : 0.f;
  w->prior = weights[E];
  return true;
}

extern "C" size_t mmvae_js_fusion_ws_floats(int B, int D) { return fusion_ws_floats(B, D); }

extern "C" int mmvae_js_fusion_fwd(const mmvae_tc_fwd_args* a, const float* weights, const float* theta, const float* eps,
                                   const int* sel, float* prior, float* kl, float* z, int E, int B, int D, int ld_in,
                                   int raw_heads, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && weights && theta && eps && sel && prior && kl && z && B > 0 && D > 0 && E > 0 && ld_in >= D);
  if (!fusion_supported(E, D)) return MMVAE_ERR_UNSUPPORTED;
  for (int e = 0; e < E; ++e) MMVAE_CHECK_ARG(a->mu[e] && a->lv[e]);
  js_weights w;
  MMVAE_CHECK_ARG(js_take_weights(weights, E, &w));
  hipLaunchKernelGGL(js_fwd_kernel, dim3(poe_blocks(B)), dim3(256), 0, (hipStream_t)stream, *a, w, theta, eps, sel, prior,
                     kl, z, E, B, D, ld_in, raw_heads ? 1 : 0);
  return mmvae_launch_status();
}

extern "C" int mmvae_js_fusion_bwd(const mmvae_tc_bwd_args* a, const float* weights, const float* theta, const float* eps,
                                   const int* sel, const float* dz, const float* dkl, float* dtheta, float* ws, int E,
                                   int B, int D, int ld_in, int raw_heads, int accumulate, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && weights && theta && eps && sel && ws && B > 0 && D > 0 && E > 0 && ld_in >= D);
  if (!fusion_supported(E, D)) return MMVAE_ERR_UNSUPPORTED;
  for (int e = 0; e < E; ++e) MMVAE_CHECK_ARG(a->mu[e] && a->lv[e] && a->dmu[e] && a->dlv[e]);
  js_weights w;
  MMVAE_CHECK_ARG(js_take_weights(weights, E, &w));
  hipLaunchKernelGGL(js_bwd_kernel, dim3(poe_blocks(B)), dim3(256), 0, (hipStream_t)stream, *a, w, theta, eps, sel, dz, dkl, ws, E, B,
                     D, ld_in, raw_heads ? 1 : 0);
  launch_theta_fold(theta, ws, dtheta, B, D, accumulate, stream);
  return mmvae_launch_status();
}
