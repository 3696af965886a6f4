// Sliced Wasserstein distances and marginal Kolmogorov-Smirnov tests (ops.swd_slices, TorchMMVAE.latent_transport and
// sliced_distances; Rabin et al. 2011, Bonneel et al. 2015, Deshpande et al. 2019): rows X (n_x, F), Y (n_y, F) fp32 are
// projected on L directions, every projection is sorted, and the two sorted lists of a direction are compared.
//   f64_tile_kernel     (f64_tile.hpp) the projections P[l][r] = sum_f dirs[l][f] row_r[f] on v_mfma_f64_16x16x4_f64: operand A the
//                       double directions, operand B the pooled fp32 rows (X's, then Y's) converted on load, the store into
//                       ws (L, n_x + n_y).  k walks in order, no K-split: a projection's bits depend on its row and its
//                       direction alone.  Axis mode (no directions) skips this launch: the sort reads column l of the rows.
//   swd_sort_kernel     one workgroup of 256 threads per (direction, set): a bitonic network over NP = the next power of two
//                       >= max(n, 256) values, +inf past n.  Thread t holds the NP / 256 values at e 256 + t in registers;
//                       a compare-exchange of stride >= 256 pairs two registers of one thread, of stride < 64 two lanes of
//                       one wave (a shuffle), of stride 64 and 128 two waves (one round trip through NP doubles of dynamic
//                       LDS: 64 KiB at n = 8192, the whole static allowance, so the kernel declares no other __shared__).
//                       Equal values (-0.0 and +0.0 among them) are never exchanged.  Sorted in place in ws.
//   swd_merge_kernel    one workgroup of 1024 threads per direction over the two sorted lists: W_1 and W_2^2 on the grid of
//                       1 / (n_x n_y) (x_(i) covers [i n_y, (i + 1) n_y), y_(j) covers [j n_x, (j + 1) n_x)), and the integer
//                       numerator of the KS statistic by binary search at the last element of every run of equal values.
// No atomics.  Every sum in a fixed order: two runs give the same bits, and a direction's outputs do not depend on L or on its
// place among the directions.
#include <math.h>

#include "f64_tile.hpp"

#define SWD_SORT_THREADS 256
#define SWD_MERGE_THREADS 1024

static bool sw_shape_ok(long n_x, long n_y, int F, int L) {
  return n_x >= 1 && n_x <= MMVAE_SWD_MAX_ROWS && n_y >= 1 && n_y <= MMVAE_SWD_MAX_ROWS && F >= 1 && F <= MMVAE_SWD_MAX_F &&
         L >= 1 && L <= MMVAE_SWD_MAX_DIRECTIONS;
}

// ---- the operands of the projection --------------------------------------------------------------------------------------------
struct SwdDirOp {      // element (l, k) = dirs[l][k]
  const double* dirs;
  int L, F;
  static constexpr bool KFAST = true;
  __device__ __forceinline__ double operator()(int l, long k) const { return (l < L && k < F) ? dirs[(size_t)l * F + k] : 0.0; }
};
struct SwdRowOp {      // element (r, k) = pooled row r (X's rows, then Y's), feature k, converted on load
  const float *X, *Y;
  long n_x, n;
  int F;
  static constexpr bool KFAST = true;
  __device__ __forceinline__ double operator()(int r, long k) const {
    if (!(r < n && k < F)) return 0.0;
    return (double)(r < n_x ? X[(size_t)r * F + k] : Y[(size_t)(r - n_x) * F + k]);
  }
};
struct SwdStore {      // ws[l][r] = v
  double* P;
  long n;
  static constexpr bool UPPER = false;
  __device__ __forceinline__ void operator()(int l, int r, double v) const { P[(size_t)l * n + r] = v; }
};

// ---- the sort: grid L, 256 threads, NP doubles of dynamic LDS --------------------------------------------------------------------
// One compare-exchange, decided alike on both sides: `lo` the value at the lower index, `hi` at the upper one; ascending runs
// exchange when hi < lo, descending ones when lo < hi -- never on equality, so no value is lost or doubled among ties.
__device__ __forceinline__ bool swd_exchange(double lo, double hi, bool asc) { return asc ? hi < lo : lo < hi; }

// rows: the set's fp32 rows (axis mode: the value of row r is rows[r F + l]) or NULL (the projections are in P already)
template <int E>
__global__ __launch_bounds__(SWD_SORT_THREADS) void swd_sort_kernel(const float* __restrict__ rows, double* __restrict__ ws,
                                                                    long n, long n_all, long offset, int F) {
  extern __shared__ double swd_lds[];
  constexpr int T = SWD_SORT_THREADS, NP = E * T;
  const int tid = threadIdx.x, l = blockIdx.x;
  double* P = ws + (size_t)l * n_all + offset;
  double v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const long idx = (long)e * T + tid;
    v[e] = idx < n ? (rows ? (double)rows[(size_t)idx * F + l] : P[idx]) : INFINITY;
  }
#pragma unroll 1
  for (int k = 2; k <= NP; k <<= 1) {
    // strides of 256 and more: two registers of this thread
#pragma unroll
    for (int je = E / 2; je > 0; je >>= 1) {
      if (je * T < k) {      // (workgroup-uniform)
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (e & je) continue;
          const bool asc = (((e * T + tid) & k) == 0);
          const double lo = v[e], hi = v[e | je];
          const bool x = swd_exchange(lo, hi, asc);
          v[e] = x ? hi : lo;
          v[e | je] = x ? lo : hi;
        }
      }
    }
    // strides 128 and 64: another wave's value, through LDS
#pragma unroll
    for (int j = T / 2; j >= 64; j >>= 1) {
      if (j < k) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e) swd_lds[e * T + tid] = v[e];
        __syncthreads();
        const bool lower = (tid & j) == 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double other = swd_lds[e * T + (tid ^ j)];
          const bool asc = (((e * T + tid) & k) == 0);
          const bool x = swd_exchange(lower ? v[e] : other, lower ? other : v[e], asc);
          v[e] = x ? other : v[e];
        }
      }
    }
    // strides below 64: another lane's value, no LDS round trip
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
      if (j < k) {
        const bool lower = (tid & j) == 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double other = __shfl_xor(v[e], j, 64);
          const bool asc = (((e * T + tid) & k) == 0);
          const bool x = swd_exchange(lower ? v[e] : other, lower ? other : v[e], asc);
          v[e] = x ? other : v[e];
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const long idx = (long)e * T + tid;
    if (idx < n) P[idx] = v[e];
  }
}

static void sw_sort(const float* rows, double* ws, long n, long n_all, long offset, int F, int L, hipStream_t s) {
  const dim3 grid(L), block(SWD_SORT_THREADS);
#define SW_SORT(E)                                                                                                       \
  hipLaunchKernelGGL((swd_sort_kernel<E>), grid, block, (size_t)(E) * SWD_SORT_THREADS * sizeof(double), s, rows, ws, n, n_all, \
                     offset, F)
  if (n <= 256) SW_SORT(1);
  else if (n <= 512) SW_SORT(2);
  else if (n <= 1024) SW_SORT(4);
  else if (n <= 2048) SW_SORT(8);
  else if (n <= 4096) SW_SORT(16);
  else SW_SORT(32);
#undef SW_SORT
}

// ---- the comparison of two sorted lists: grid L, 1024 threads ------------------------------------------------------------------------
__device__ __forceinline__ long long swd_max(long long a, long long b) { return a > b ? a : b; }

// #{v <= t} of a sorted list
__device__ __forceinline__ long swd_count_le(const double* __restrict__ v, long n, double t) {
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (v[mid] <= t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// W_p^p = (1 / N) sum_i sum_j len_ij |x_(i) - y_(j)|^p, N = n_x n_y, len_ij the overlap of [i n_y, (i + 1) n_y) and
// [j n_x, (j + 1) n_x).  Thread t adds the terms of i = t, t + 1024, ... in order, j ascending within i; the 1024 partials
// are added by the tree red[t] += red[t + o], o = 512, 256, ... 1.  ks = max over the pooled values t of |n_y #{x <= t} -
// n_x #{y <= t}|, taken at the last element of every run of equal values of either list: an integer maximum.
__global__ __launch_bounds__(SWD_MERGE_THREADS) void swd_merge_kernel(const double* __restrict__ ws, double* __restrict__ w,
                                                                      long long* __restrict__ ks, long n_x, long n_y) {
  __shared__ double red1[SWD_MERGE_THREADS], red2[SWD_MERGE_THREADS];
  __shared__ long long redk[SWD_MERGE_THREADS];
  const int tid = threadIdx.x, l = blockIdx.x;
  const double* xs = ws + (size_t)l * (n_x + n_y);
  const double* ys = xs + n_x;
  double s1 = 0.0, s2 = 0.0;
  long long best = 0;
  for (long i = tid; i < n_x; i += SWD_MERGE_THREADS) {
    const double x = xs[i];
    const long a = i * n_y, b = a + n_y;      // x_(i) covers [a, b)
    for (long j = a / n_x; j < n_y && j * n_x < b; ++j) {
      const long c = j * n_x, from = a > c ? a : c, to = b < c + n_x ? b : c + n_x;
      const double len = (double)(to - from), d = fabs(x - ys[j]);
      s1 += len * d;
      s2 += len * (d * d);
    }
    if (i == n_x - 1 || !(xs[i + 1] == x)) {
      const long long v = (long long)n_y * (i + 1) - (long long)n_x * swd_count_le(ys, n_y, x);
      best = swd_max(best, v < 0 ? -v : v);
    }
  }
  for (long j = tid; j < n_y; j += SWD_MERGE_THREADS) {
    const double y = ys[j];
    if (j == n_y - 1 || !(ys[j + 1] == y)) {
      const long long v = (long long)n_y * swd_count_le(xs, n_x, y) - (long long)n_x * (j + 1);
      best = swd_max(best, v < 0 ? -v : v);
    }
  }
  red1[tid] = s1;
  red2[tid] = s2;
  redk[tid] = best;
  __syncthreads();
  for (int o = SWD_MERGE_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red1[tid] += red1[tid + o];
      red2[tid] += red2[tid + o];
      redk[tid] = swd_max(redk[tid], redk[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double N = (double)n_x * (double)n_y;
    w[2 * (size_t)l + 0] = red1[0] / N;
    w[2 * (size_t)l + 1] = red2[0] / N;
    ks[l] = redk[0];
  }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" size_t mmvae_swd_ws_doubles(long n_x, long n_y, int F, int L) {
  if (!sw_shape_ok(n_x, n_y, F, L)) return 0;
  return (size_t)L * (size_t)(n_x + n_y);
}

extern "C" int mmvae_swd_slices(const float* X, const float* Y, const double* dirs, double* ws, double* w, long long* ks,
                                long n_x, long n_y, int F, int L, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && Y && ws && w && ks);
  if (!sw_shape_ok(n_x, n_y, F, L) || (!dirs && L != F)) return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const long n = n_x + n_y;
  if (dirs) f64_launch_tiles(SwdDirOp{dirs, L, F}, SwdRowOp{X, Y, n_x, n, F}, SwdStore{ws, n}, L, (int)n, (long)F, s);
  sw_sort(dirs ? nullptr : X, ws, n_x, n, 0, F, L, s);
  sw_sort(dirs ? nullptr : Y, ws, n_y, n, n_x, F, L, s);
  hipLaunchKernelGGL(swd_merge_kernel, dim3(L), dim3(SWD_MERGE_THREADS), 0, s, ws, w, ks, n_x, n_y);
  return mmvae_launch_status();
}
