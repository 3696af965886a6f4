// The fp64 MFMA: its one slab step (f64_mfma_slab: cca.hip's score, pair_tile.hpp's walker and the tile routine below) and the
// tile routine shared by frechet.hip (moments, mmvae_f64_gemm, the distance) and cca.hip (mmvae_f64_gemm_ld).
// C(i, j) = sum_k a(i, k) b(j, k) over a 64 x 64 tile of an (M, N) result.  Operand functors return 0 outside the matrix; KFAST
// says whether k is the contiguous index of the operand's memory (which index the staging threads walk first).
// v_mfma_f64_16x16x4_f64: lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one double each; it holds
// D[row = (l >> 4) + 4 r][col = l & 15] in register r (NOT the f32 forms' row = 4 (l >> 4) + r).
#pragma once
#include "common.hpp"

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define FR_TILE 64            // C tile of a workgroup
#define FR_KT 16              // k-depth of a staged tile
#define FR_LD (FR_TILE + 2)   // LDS row stride in doubles

// The one place the MFMA is issued.  A slab staged in LDS as Rs[k][row of the tile], Cs[k][column of the tile], KT deep, row
// stride LD doubles: the wave at (wm, wn) of the 64 x 64 tile adds the slab's products to its 32 x 32 block, acc[mi][ni] the
// 16 x 16 block at (wm + 16 mi, wn + 16 ni); lr = lane & 15, lk = lane >> 4.  k runs in order.  UNROLL: the unroll factor of
// the loop over k (KT / 4: all of it), the caller's choice of code size and registers.
template <int KT, int LD, int UNROLL>
__device__ __forceinline__ void f64_mfma_slab(double (*Rs)[LD], double (*Cs)[LD], int wm, int wn, int lr, int lk,
                                              f64x4 (&acc)[2][2]) {
#pragma unroll UNROLL
  for (int k4 = 0; k4 < KT; k4 += 4) {
    double rv[2], cv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      rv[t] = Rs[k4 + lk][wm + 16 * t + lr];
      cv[t] = Cs[k4 + lk][wn + 16 * t + lr];
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(rv[mi], cv[ni], acc[mi][ni], 0, 0, 0);
  }
}

template <class OpA, class OpB, class Store>
__global__ __launch_bounds__(256) void f64_tile_kernel(OpA a, OpB b, Store st, int M, int N, long K) {
  __shared__ double As[FR_KT][FR_LD], Bs[FR_KT][FR_LD];
  if (Store::UPPER && blockIdx.x < blockIdx.y) return;      // (workgroup-uniform, before any barrier)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.y * FR_TILE, j0 = blockIdx.x * FR_TILE;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, lr = lane & 15, lk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (long k0 = 0; k0 < K; k0 += FR_KT) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < FR_TILE * FR_KT / 256; ++e) {
      const int idx = tid + 256 * e;
      const int ia = OpA::KFAST ? idx >> 4 : idx & 63, ka = OpA::KFAST ? idx & 15 : idx >> 6;
      As[ka][ia] = a(i0 + ia, k0 + ka);
      const int ib = OpB::KFAST ? idx >> 4 : idx & 63, kb = OpB::KFAST ? idx & 15 : idx >> 6;
      Bs[kb][ib] = b(j0 + ib, k0 + kb);
    }
    __syncthreads();
    f64_mfma_slab<FR_KT, FR_LD, FR_KT / 4>(As, Bs, wm, wn, lr, lk, acc);
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wm + 16 * mi + lk + 4 * r, j = j0 + wn + 16 * ni + lr;
        if (i < M && j < N) st(i, j, acc[mi][ni][r]);
      }
}

// grid: ceil(N / 64) x ceil(M / 64) workgroups of 256 threads
template <class OpA, class OpB, class Store>
static void f64_launch_tiles(OpA a, OpB b, Store st, int M, int N, long K, hipStream_t s) {
  hipLaunchKernelGGL((f64_tile_kernel<OpA, OpB, Store>), dim3((N + FR_TILE - 1) / FR_TILE, (M + FR_TILE - 1) / FR_TILE),
                     dim3(256), 0, s, a, b, st, M, N, K);
}
