// The counter-based device noise streams (mmvae_randn, mmvae_rand_laplace) as per-element device functions, shared by
// the kernels that draw their noise in place (latent.hip, loglik.hip) and the generator kernels themselves.
// State = {seed, call counter, ticket}; a draw is keyed by (seed, call counter), the two families by distinct constants.
#pragma once
#include "common.hpp"

// element e of the counter-based standard-normal stream `key` (see randn_kernel: Box-Muller over the hash pair of
// element pair e >> 1; the even element takes the cosine branch)
__device__ __forceinline__ uint32_t randn_key(const uint32_t* __restrict__ state) {
  return drop_fmix(state[0] ^ (state[1] * 0x9E3779B1u) ^ 0x632BE5ABu);
}
__device__ __forceinline__ float randn_elem(uint32_t key, long e) {
  const long i = e >> 1;
  const uint32_t h1 = drop_fmix(key + (uint32_t)(2 * i) * 0x9E3779B1u);
  const uint32_t h2 = drop_fmix(key + (uint32_t)(2 * i + 1) * 0x9E3779B1u);
  const float u1 = ((float)(h1 >> 8) + 1.0f) * (1.0f / 16777216.0f);   // (0, 1]
  const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);            // [0, 1)
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  return (e & 1) ? r * sn : r * cs;
}
// element e of the standard-Laplace stream (see rand_laplace_kernel): e = -sign(u) log1p(-|u|), u ~ U(-1, 1)
__device__ __forceinline__ uint32_t rand_laplace_key(const uint32_t* __restrict__ state) {
  return drop_fmix(state[0] ^ (state[1] * 0x9E3779B1u) ^ 0x1B873593u);
}
__device__ __forceinline__ float rand_laplace_elem(uint32_t key, long e) {
  const uint32_t h = drop_fmix(key + (uint32_t)e * 0x9E3779B1u);
  const float u = ((float)(h >> 9) + 0.5f) * (1.0f / 4194304.0f) - 1.0f;      // (-1, 1) exactly: never 0 or +-1
  const float m = -log1pf(-fabsf(u));
  return u < 0.f ? -m : m;
}
// the last workgroup of a launch that consumed the stream advances its counter
__device__ __forceinline__ void randn_advance(uint32_t* __restrict__ state) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t ticket = atomicAdd(state + 2, 1u);
    if (ticket == gridDim.x - 1) {
      state[2] = 0u;
      state[1] += 1u;
    }
  }
}
