// MMVAE+ (Palumbo, Daunhawer, Vogt, ICLR 2023), K = 1, for gfx950: every one of the E encoders emits W = D + P columns --
// [0, D) its SHARED posterior q_m^u, [D, W) its PRIVATE posterior q_m^w --, and one launch each way does the whole latent
// side of a step: one reparameterised sample (u_m, w_m) per modality, the auxiliary private draws s eps_a[n][m] every OTHER
// decoder n gets in place of w_m, every decoder's whole input batch z[n] (E B, W), the one-sample estimate of the shared
// posterior's KL to the uniform mixture of all E (mixture_rows.hpp, shared with mixprior.hip), the closed-form KLs of
// the shared posterior to N(0, sp) and of the private one to N(0, 1), and the responsibilities.  The frame is
// latent_rows.hpp's: one wavefront per sample, lanes over the columns in POE_SLOTS slots of 64 -- the shared columns in
// one sweep, the private ones in a second --, wave-shuffle row sums; no atomics and no in-launch election: every sum is
// taken in one fixed order.
//
// Head e is [mu_e | lv_e], W columns each, rows ld_in floats apart; raw heads: lv = softmax(u, -1) + 1e-6 over all W
// columns, so the shared and the private columns share one normaliser and, backward, one dot product.  With sigma = lv,
// sp = softmax(theta) D, u_m = mu_m^u + sigma_m^u eps_u[m], w_m = mu_m^w + sigma_m^w eps_w[m]:
//   z[n] row m B + b = [u_m | w_m]  (n == m)     [u_m | s eps_a[n][m]]  (n != m)
//   kl row m       = log q_m^u(u_m) - log (1/E) sum_j q_j^u(u_m)        (mixture_rows.hpp: D_mj, formed from differences)
//   kl row E + m   = sum_d KL(q_m^u || N(0, sp))
//   kl row 2E + m  = sum_p KL(q_m^w || N(0, 1))
//   resp[m][j]     = softmax_j D_mj
// Backward: the gradient of u_m is the sum over n = 0 .. E-1, in that order, of columns [0, D) of row block m of dz[n];
// the gradient of w_m is columns [D, W) of row block m of dz[m] alone (the auxiliary draws are noise).  The pair terms are
// mixture_rows.hpp's; the private columns add  dmu = gw + g'' mu,  dsg = gw eps_w + g'' (sigma - 1 / sigma),  g'' = dkl[2E + m].
// The prior gradient is split at its cancellation (the end of mmplus_bwd_kernel).
#include <cmath>

#include "common.hpp"
#include "mixture_rows.hpp"

__global__ __launch_bounds__(256) void mmplus_fwd_kernel(mmvae_mmplus_fwd_args a, const float* __restrict__ theta,
                                                         const float* __restrict__ eps_u, const float* __restrict__ eps_w,
                                                         const float* __restrict__ eps_a, float aux, float* __restrict__ kl,
                                                         float* __restrict__ resp, int E, int B, int D, int P, int ld, int raw) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int W = D + P;
  float sp[POE_SLOTS], sm[POE_SLOTS];
  prior_sigma(theta, D, lane, sp, sm);
  const float logE = logf((float)E);
  for (int b = wave; b < B; b += nwaves) {
    float dl[MMVAE_MAX_EXPERTS][MMVAE_MAX_EXPERTS], ks[MMVAE_MAX_EXPERTS], kw[MMVAE_MAX_EXPERTS];
#pragma unroll
    for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {
      ks[m] = kw[m] = 0.f;
#pragma unroll
      for (int j = 0; j < MMVAE_MAX_EXPERTS; ++j) dl[m][j] = 0.f;
    }
    float umx[MMVAE_MAX_EXPERTS], uinv[MMVAE_MAX_EXPERTS];
    if (raw) raw_head_stats(a.lv, E, (size_t)b * ld, W, lane, umx, uinv);
    // ---- the shared columns: mixprior.hip's sweep around mixture_rows.hpp; u_m goes to row block m of EVERY decoder's batch
#pragma unroll
    for (int s = 0; s < POE_SLOTS; ++s) {
      const int d = lane + 64 * s;
      if (d < D) {
        const size_t oi = (size_t)b * ld + d;  // strided head tensors
        float mu[MMVAE_MAX_EXPERTS], sg[MMVAE_MAX_EXPERTS], ep[MMVAE_MAX_EXPERTS];
#pragma unroll
        for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) {
          if (e >= E) continue;
          mu[e] = a.mu[e][oi];
          sg[e] = a.lv[e][oi];
          if (raw) sg[e] = raw_head_scale(sg[e], umx[e], uinv[e]);
          ep[e] = eps_u[((size_t)e * B + b) * D + d];
          const float zu = mu[e] + sg[e] * ep[e];
          const size_t oz = ((size_t)e * B + b) * W + d;
#pragma unroll
          for (int n = 0; n < MMVAE_MAX_EXPERTS; ++n)
            if (n < E) a.z[n][oz] = zu;
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
    // ---- the private columns: w_m to decoder m's own block, a scaled auxiliary draw to every other decoder's
#pragma unroll
    for (int s = 0; s < POE_SLOTS; ++s) {
      const int p = lane + 64 * s;
      if (p < P) {
        const size_t oi = (size_t)b * ld + D + p;
#pragma unroll
        for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {
          if (m >= E) continue;
          const float mu = a.mu[m][oi];
          float sg = a.lv[m][oi];
          if (raw) sg = raw_head_scale(sg, umx[m], uinv[m]);
          const size_t oz = ((size_t)m * B + b) * W + D + p;
#pragma unroll
          for (int n = 0; n < MMVAE_MAX_EXPERTS; ++n) {
            if (n >= E) continue;
            a.z[n][oz] = n == m ? mu + sg * eps_w[((size_t)m * B + b) * P + p]
                                : aux * eps_a[(((size_t)n * E + m) * B + b) * P + p];
          }
          kw[m] += kl_elem(mu, sg, 1.0f);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {
      if (m >= E) continue;
      const float kstd = wave_sum(ks[m]);
      const float kprv = wave_sum(kw[m]);
      mix_row_finish(dl, m, E, B, b, lane, logE, kl, resp);
      if (lane == 0) {
        kl[(size_t)(E + m) * B + b] = kstd;
        kl[(size_t)(2 * E + m) * B + b] = kprv;
      }
    }
  }
}

// a.dz[n] / dkl == NULL: that upstream gradient is absent and counts as zeros
__global__ __launch_bounds__(256) void mmplus_bwd_kernel(mmvae_mmplus_bwd_args a, const float* __restrict__ theta,
                                                         const float* __restrict__ eps_u, const float* __restrict__ eps_w,
                                                         const float* __restrict__ resp, const float* __restrict__ dkl,
                                                         float* __restrict__ ws, float* __restrict__ dtheta, int accumulate,
                                                         int E, int B, int D, int P, int ld, int raw) {
  __shared__ float part[4][64 * POE_SLOTS];
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int W = D + P;
  float sp[POE_SLOTS], sm[POE_SLOTS], dsp[POE_SLOTS];
  prior_sigma(theta, D, lane, sp, sm);
#pragma unroll
  for (int s = 0; s < POE_SLOTS; ++s) dsp[s] = 0.f;
  for (int b = wave; b < B; b += nwaves) {
    float c[MMVAE_MAX_EXPERTS][MMVAE_MAX_EXPERTS], gs[MMVAE_MAX_EXPERTS], gp[MMVAE_MAX_EXPERTS];
    mix_upstream(dkl, resp, E, B, b, c, gs);
#pragma unroll
    for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m)
      if (m < E) gp[m] = dkl ? dkl[(size_t)(2 * E + m) * B + b] : 0.f;
    float umx[MMVAE_MAX_EXPERTS], uinv[MMVAE_MAX_EXPERTS], udot[MMVAE_MAX_EXPERTS];
#pragma unroll
    for (int e = 0; e < MMVAE_MAX_EXPERTS; ++e) udot[e] = 0.f;
    if (raw) raw_head_stats(a.lv, E, (size_t)b * ld, W, lane, umx, uinv);
    // ---- the shared columns
#pragma unroll
    for (int s = 0; s < POE_SLOTS; ++s) {
      const int d = lane + 64 * s;
      if (d < D) {
        const size_t oi = (size_t)b * ld + d;  // strided head tensors
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
          ep[e] = eps_u[((size_t)e * B + b) * D + d];
          inv[e] = 1.0f / sg[e];
          // u_e is read by every decoder: its gradient is their sum, decoder 0 first
          const size_t oz = ((size_t)e * B + b) * W + d;
          float gz = 0.f;
#pragma unroll
          for (int n = 0; n < MMVAE_MAX_EXPERTS; ++n)
            if (n < E && a.dz[n]) gz += a.dz[n][oz];
          dmu[e] = gz + gs[e] * (mu[e] * r);
          dsg[e] = gz * ep[e] + gs[e] * (sg[e] * r - inv[e]);
          dspv -= gs[e] * (((sg[e] * sg[e] + mu[e] * mu[e]) * r) / sp[s]);      // (without the 1: see the end of the kernel)
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
    // ---- the private columns: w_m is read by decoder m alone
#pragma unroll
    for (int s = 0; s < POE_SLOTS; ++s) {
      const int p = lane + 64 * s;
      if (p < P) {
        const size_t oi = (size_t)b * ld + D + p;
#pragma unroll
        for (int m = 0; m < MMVAE_MAX_EXPERTS; ++m) {
          if (m >= E) continue;
          const float mu = a.mu[m][oi];
          float sg = a.lv[m][oi];
          if (raw) sg = raw_head_scale(sg, umx[m], uinv[m]);
          const float gz = a.dz[m] ? a.dz[m][((size_t)m * B + b) * W + D + p] : 0.f;
          const float dsg = gz * eps_w[((size_t)m * B + b) * P + p] + gp[m] * (sg - 1.0f / sg);
          a.dmu[m][oi] = gz + gp[m] * mu;
          a.dlv[m][oi] = dsg;
          udot[m] += (sg - 1e-6f) * dsg;
        }
      }
    }
    // raw heads: one softmax over all W columns, so one dot product per head over both sweeps
    if (raw) raw_head_bwd(a.lv, a.dlv, E, (size_t)b * ld, W, lane, umx, uinv, udot);
  }
  // d kl_u / d sp = g' (1 - q) / sp, q = (sigma^2 + mu^2) / sp^2.  The fold maps the 1's, G = sum g' over rows and experts, to
  // G (1 - sp_d): a difference of sums of size G that is ~G q wherever the posteriors are narrow against the prior (theta = 0:
  // exactly 0), so the partial rows would have to carry G to the precision of G q (measured on the MNIST + SVHN towers,
  // means pulled together: 1e-4 of the gradient's maximum lost).  The rows carry the q part alone, and workgroup 0 leaves
  // G (1 - sp_d) in dtheta, where the fold -- always accumulating -- adds its part: the same sum, every term at its own size.
  if (blockIdx.x == 0 && dtheta) {
    float g = 0.f;
    if (dkl)
      for (int i = threadIdx.x; i < E * B; i += 256) g += dkl[(size_t)E * B + i];
    g = block_sum_256(g, red);
    const int w = threadIdx.x >> 6;      // thread t holds column t = lane + 64 w in slot w
    const float spd = w == 0 ? sp[0] : w == 1 ? sp[1] : w == 2 ? sp[2] : sp[3];
    if ((int)threadIdx.x < D) {
      const float c = g * (1.0f - spd);
      dtheta[threadIdx.x] = accumulate ? dtheta[threadIdx.x] + c : c;
    }
  }
  prior_grad_row(dsp, part, ws, D, lane);
}

static inline bool mmplus_supported(int E, int D, int P) {
  return E >= 1 && D >= 1 && P >= 1 && D + P <= 64 * POE_SLOTS && fusion_supported(E, D);
}

extern "C" size_t mmvae_mmplus_ws_floats(int B, int D, int P) {
  return mmplus_supported(1, D, P) ? fusion_ws_floats(B, D) : 0;
}

extern "C" int mmvae_mmplus_fwd(const mmvae_mmplus_fwd_args* a, const float* theta, const float* eps_u, const float* eps_w,
                                const float* eps_a, float aux_scale, float* kl, float* resp, int E, int B, int D, int P,
                                int ld_in, int raw_heads, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && theta && eps_u && eps_w && kl && resp && B > 0);
  if (!mmplus_supported(E, D, P)) return MMVAE_ERR_UNSUPPORTED;
  MMVAE_CHECK_ARG(ld_in >= D + P && (eps_a || E == 1) && std::isfinite(aux_scale) && aux_scale > 0.f);
  for (int e = 0; e < E; ++e) MMVAE_CHECK_ARG(a->mu[e] && a->lv[e] && a->z[e]);
  hipLaunchKernelGGL(mmplus_fwd_kernel, dim3(poe_blocks(B)), dim3(256), 0, (hipStream_t)stream, *a, theta, eps_u, eps_w,
                     eps_a, aux_scale, kl, resp, E, B, D, P, ld_in, raw_heads ? 1 : 0);
  return mmvae_launch_status();
}

extern "C" int mmvae_mmplus_bwd(const mmvae_mmplus_bwd_args* a, const float* theta, const float* eps_u, const float* eps_w,
                                const float* resp, const float* dkl, float* dtheta, float* ws, int E, int B, int D, int P,
                                int ld_in, int raw_heads, int accumulate, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && theta && eps_u && eps_w && resp && ws && B > 0);
  if (!mmplus_supported(E, D, P)) return MMVAE_ERR_UNSUPPORTED;
  MMVAE_CHECK_ARG(ld_in >= D + P);
  for (int e = 0; e < E; ++e) MMVAE_CHECK_ARG(a->mu[e] && a->lv[e] && a->dmu[e] && a->dlv[e]);
  hipLaunchKernelGGL(mmplus_bwd_kernel, dim3(poe_blocks(B)), dim3(256), 0, (hipStream_t)stream, *a, theta, eps_u, eps_w, resp,
                     dkl, ws, dtheta, accumulate ? 1 : 0, E, B, D, P, ld_in, raw_heads ? 1 : 0);
  launch_theta_fold(theta, ws, dtheta, B, D, 1, stream);      // (onto what workgroup 0 left there)
  return mmvae_launch_status();
}
