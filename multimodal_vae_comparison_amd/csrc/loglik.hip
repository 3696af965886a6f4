// Held-out log-likelihood estimation (TorchMMVAE.estimate_log_likelihood): the latent half of the K-sample
// importance-sampled bound, forward only.
//   mmvae_mix_ksample_logw_fwd: stratified draws from the mixture proposal q(z | x_G) = (1/C) sum_c q_c(z) and
//     lw0[k,b] = sum_d log p(z) - log((1/C) sum_c exp sum_d log q_c(z))
//   mmvae_lme_update / mmvae_lme_finish: streaming log-sum-exp over the K axis, fp64 state, for the joint weights
//     lw0 + sum_m ll_m and every conditional ll_m at once.
// The decoders and the likelihood row sums between the two are the existing kernels.
#include "common.hpp"
#include "noise.hpp"

#define HALF_LOG_2PI_F 0.9189385332046727f

// softmax(theta) * D of the lane's coordinates d = lane + 64 s (TorchMMVAE.pz_params); 0 beyond D
template <int SLOTS>
__device__ __forceinline__ void mix_prior_scale(const float* __restrict__ theta, int D, int lane, float sp[SLOTS]) {
  float mx = -INFINITY;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int d = lane + 64 * s;
    if (d < D) mx = fmaxf(mx, theta[d]);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int d = lane + 64 * s;
    sp[s] = d < D ? expf(theta[d] - mx) : 0.f;
    sum += sp[s];
  }
  sum = wave_sum(sum);
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) sp[s] = sp[s] / sum * (float)D;
}

// log density of one coordinate WITHOUT its normaliser: t = (z - loc) / scale
__device__ __forceinline__ float mix_logq_var(float t, bool laplace) { return laplace ? -fabsf(t) : -0.5f * t * t; }
// ... and the normaliser: -log(scale) - log sqrt(2 pi)  |  -log(2 scale)
__device__ __forceinline__ float mix_logq_const(float scale, bool laplace) {
  return laplace ? -logf(2.0f * scale) : -logf(scale) - HALF_LOG_2PI_F;
}

// ---------------------------------------------------------------------------------------------
// One wave per (sample b, slice of the Kc draws); lanes over d (lane + 64 s, SLOTS <= 4: D <= 256).  The wave reads
// the C component rows of b ONCE -- loc, scale and 1 / scale stay in registers, the normalisers' row sums are folded
// into one scalar per component -- and then walks its draws k = slice, slice + n_slices, ...: per draw one eps read
// (or one generator element), one z store, C + 1 wave reductions and a C-term log-sum-exp.
// Draw k0 + k comes from component (k0 + k) % C.  Generator: element (k0 + k) B D + b D + d of the current draw of
// the component's family, so a chunk [k0, k0 + Kc) of a larger draw is reproducible; `advance` != 0 lets the last
// workgroup bump the call counter (the caller sets it on the last chunk of a draw).
// CP = C rounded up to a power of two: the component loops unroll to CP with c < C as a wave-uniform predicate.
// ---------------------------------------------------------------------------------------------
template <int SLOTS, int CP>
__global__ __launch_bounds__(256) void mix_ksample_logw_kernel(const float* __restrict__ comps, unsigned lap_mask,
                                                               const float* __restrict__ theta,
                                                               const float* __restrict__ prior_loc, int prior_laplace,
                                                               const float* __restrict__ eps, uint32_t* rng, int advance,
                                                               float* __restrict__ z, float* __restrict__ lw0, int C,
                                                               int Kc, int k0, int B, int D, int n_slices) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = (int)(w / n_slices), slice = (int)(w - (long)b * n_slices);
  if (b < B) {
    const uint32_t nkey = rng ? randn_key(rng) : 0u, lkey = rng ? rand_laplace_key(rng) : 0u;
    float ploc[SLOTS], pinv[SLOTS];
    mix_prior_scale<SLOTS>(theta, D, lane, pinv);
    float pconst = 0.f;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int d = lane + 64 * s;
      const bool in = d < D;
      ploc[s] = (in && prior_loc) ? prior_loc[d] : 0.f;
      if (in) pconst += mix_logq_const(pinv[s], prior_laplace != 0);
      pinv[s] = in ? 1.0f / pinv[s] : 0.f;      // (a coordinate beyond D adds exactly 0 to every sum)
    }
    pconst = wave_sum(pconst);
    float loc[CP][SLOTS], sc[CP][SLOTS], inv[CP][SLOTS], qconst[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int d = lane + 64 * s;
        const bool in = c < C && d < D;
        const float* __restrict__ row = comps + ((size_t)(in ? c : 0) * B + b) * 2 * D;
        loc[c][s] = in ? row[d] : 0.f;
        sc[c][s] = in ? row[D + d] : 0.f;
        inv[c][s] = in ? 1.0f / sc[c][s] : 0.f;
        if (in) acc += mix_logq_const(sc[c][s], (lap_mask >> c) & 1u);
      }
      qconst[c] = c < C ? wave_sum(acc) : 0.f;
    }
    const float log_c = logf((float)C);
    for (int k = slice; k < Kc; k += n_slices) {
      const int kg = k0 + k, sel = kg % C;
      const bool sel_lap = (lap_mask >> sel) & 1u;
      const size_t off = ((size_t)k * B + b) * D;
      const long goff = ((long)kg * B + b) * D;
      float lp = 0.f, lq[CP];
#pragma unroll
      for (int c = 0; c < CP; ++c) lq[c] = 0.f;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int d = lane + 64 * s;
        float m = 0.f, sg = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          m = c == sel ? loc[c][s] : m;
          sg = c == sel ? sc[c][s] : sg;
        }
        float e = 0.f;
        if (d < D) e = eps ? eps[off + d] : (sel_lap ? rand_laplace_elem(lkey, goff + d) : randn_elem(nkey, goff + d));
        const float zv = m + sg * e;
        if (d < D) z[off + d] = zv;
        lp += mix_logq_var((zv - ploc[s]) * pinv[s], prior_laplace != 0);
#pragma unroll
        for (int c = 0; c < CP; ++c)
          if (c < C) lq[c] += mix_logq_var((zv - loc[c][s]) * inv[c][s], (lap_mask >> c) & 1u);
      }
      lp = wave_sum(lp) + pconst;
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        if (c < C) {
          lq[c] = wave_sum(lq[c]) + qconst[c];
          mx = fmaxf(mx, lq[c]);
        }
      }
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) se += expf(lq[c] - mx);
      if (lane == 0) lw0[(size_t)k * B + b] = lp - (mx + logf(se) - log_c);
    }
  }
  if (rng && advance) randn_advance(rng);
}

template <int SLOTS>
static void mix_launch(int CP, dim3 grid, hipStream_t st, const float* comps, unsigned lap_mask, const float* theta,
                       const float* prior_loc, int prior_laplace, const float* eps, uint32_t* rng, int advance, float* z,
                       float* lw0, int C, int Kc, int k0, int B, int D, int n_slices) {
#define MIX_GO(cp)                                                                                                   \
  hipLaunchKernelGGL((mix_ksample_logw_kernel<SLOTS, cp>), grid, dim3(256), 0, st, comps, lap_mask, theta, prior_loc, \
                     prior_laplace, eps, rng, advance, z, lw0, C, Kc, k0, B, D, n_slices)
  switch (CP) {
    case 1: MIX_GO(1); break;
    case 2: MIX_GO(2); break;
    case 4: MIX_GO(4); break;
    default: MIX_GO(8); break;
  }
#undef MIX_GO
}

extern "C" int mmvae_mix_ksample_logw_fwd(const float* comps, unsigned laplace_mask, const float* theta,
                                          const float* prior_loc, int prior_laplace, const float* eps,
                                          uint32_t* rng_state, int advance, float* z, float* lw0, int C, int Kc, int k0,
                                          int B, int D, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(comps && theta && z && lw0 && (eps || rng_state) && Kc > 0 && k0 >= 0 && B > 0 && C > 0 && D > 0);
  if (C > MMVAE_MIX_MAX_COMPONENTS || D > 256) return MMVAE_ERR_UNSUPPORTED;
  // enough waves to fill the chip (256 CUs x 8 resident waves) while every wave still amortises its component rows
  int n_slices = (4096 + B - 1) / B;
  if (n_slices > Kc) n_slices = Kc;
  const long waves = (long)B * n_slices;
  const dim3 grid((unsigned)((waves + 3) / 4));
  const int CP = C <= 1 ? 1 : (C <= 2 ? 2 : (C <= 4 ? 4 : 8));
  hipStream_t st = (hipStream_t)stream;
  if (D <= 64)
    mix_launch<1>(CP, grid, st, comps, laplace_mask, theta, prior_loc, prior_laplace, eps, rng_state, advance, z, lw0, C,
                  Kc, k0, B, D, n_slices);
  else if (D <= 128)
    mix_launch<2>(CP, grid, st, comps, laplace_mask, theta, prior_loc, prior_laplace, eps, rng_state, advance, z, lw0, C,
                  Kc, k0, B, D, n_slices);
  else
    mix_launch<4>(CP, grid, st, comps, laplace_mask, theta, prior_loc, prior_laplace, eps, rng_state, advance, z, lw0, C,
                  Kc, k0, B, D, n_slices);
  return mmvae_launch_status();
}

// ---------------------------------------------------------------------------------------------
// Streaming log-sum-exp.  state (doubles): (R, 3, B) with R = 1 + n_rows; row 0 = the joint weights
// w = lw0 + sum_{m in joint_mask} ll[m], row 1 + m = ll[m].  Per (row, b): [0] running maximum (-inf when empty),
// [1] sum exp(w - max), [2] sum exp(2 (w - max)).  One thread per sample b walks the Kc terms of the chunk in k order
// (coalesced over b), so the result does not depend on the launch geometry.
// ---------------------------------------------------------------------------------------------
struct LmeAcc {
  double mx, s1, s2;
  __device__ __forceinline__ void add(double w) {
    if (w > mx) {      // (also the first term: exp(-inf) = 0)
      const double r = exp(mx - w);
      s1 = s1 * r + 1.0;
      s2 = s2 * r * r + 1.0;
      mx = w;
    } else if (w == mx) {      // (covers w = mx = -inf: no NaN from inf - inf)
      s1 += 1.0;
      s2 += 1.0;
    } else {
      const double r = exp(w - mx);
      s1 += r;
      s2 += r * r;
    }
  }
};

__global__ __launch_bounds__(256) void lme_update_kernel(double* __restrict__ state, const float* __restrict__ lw0,
                                                         mmvae_lme_rows rows, int n_rows, unsigned joint_mask, int Kc,
                                                         int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  LmeAcc acc[1 + MMVAE_MOE_MAX_MODS];
#pragma unroll
  for (int r = 0; r <= MMVAE_MOE_MAX_MODS; ++r) {
    if (r <= n_rows) {
      double* s = state + (size_t)r * 3 * B;
      acc[r].mx = s[b];
      acc[r].s1 = s[B + b];
      acc[r].s2 = s[2 * (size_t)B + b];
    }
  }
  for (int k = 0; k < Kc; ++k) {
    const size_t i = (size_t)k * B + b;
    double w = (double)lw0[i];
#pragma unroll
    for (int m = 0; m < MMVAE_MOE_MAX_MODS; ++m) {
      if (m < n_rows) {
        const double l = (double)rows.ll[m][i];
        acc[1 + m].add(l);
        if ((joint_mask >> m) & 1u) w += l;
      }
    }
    acc[0].add(w);
  }
#pragma unroll
  for (int r = 0; r <= MMVAE_MOE_MAX_MODS; ++r) {
    if (r <= n_rows) {
      double* s = state + (size_t)r * 3 * B;
      s[b] = acc[r].mx;
      s[B + b] = acc[r].s1;
      s[2 * (size_t)B + b] = acc[r].s2;
    }
  }
}

// out (R, B): log-mean-exp over the K terms folded so far;  ess (B): (sum w)^2 / sum w^2 of the joint weights (row 0)
__global__ __launch_bounds__(256) void lme_finish_kernel(const double* __restrict__ state, double* __restrict__ out,
                                                         double* __restrict__ ess, int R, long K, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R * B) return;
  const int r = i / B, b = i - r * B;
  const double* s = state + (size_t)r * 3 * B;
  out[i] = s[b] + log(s[B + b]) - log((double)K);
  if (r == 0) ess[b] = s[B + b] * s[B + b] / s[2 * (size_t)B + b];
}

extern "C" int mmvae_lme_update(double* state, const float* lw0, const mmvae_lme_rows* rows, int n_rows,
                                unsigned joint_mask, int Kc, int B, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && lw0 && rows && n_rows >= 0 && Kc > 0 && B > 0);
  if (n_rows > MMVAE_MOE_MAX_MODS) return MMVAE_ERR_UNSUPPORTED;
  for (int m = 0; m < n_rows; ++m) MMVAE_CHECK_ARG(rows->ll[m]);
  hipLaunchKernelGGL(lme_update_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, lw0, *rows,
                     n_rows, joint_mask, Kc, B);
  return mmvae_launch_status();
}

extern "C" int mmvae_lme_finish(const double* state, double* out, double* ess, int n_rows, long K, int B,
                                mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && out && ess && n_rows >= 0 && K > 0 && B > 0);
  if (n_rows > MMVAE_MOE_MAX_MODS) return MMVAE_ERR_UNSUPPORTED;
  const int n = (1 + n_rows) * B;
  hipLaunchKernelGGL(lme_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, out, ess,
                     1 + n_rows, K, B);
  return mmvae_launch_status();
}
