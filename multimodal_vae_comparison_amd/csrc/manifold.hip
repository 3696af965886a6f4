// k-nearest-neighbour manifold estimates of generated images (TorchMMVAE.manifold_metrics): improved precision and recall
// (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020), from three kinds of pair-distance pass over two
// feature sets, squared distances in double: d^2(x, y) = max(0, (|x|^2 + |y|^2) - 2 x . y).
//   mf_sqnorms_kernel   |x_i|^2 summed in double in feature order, one thread per row
//   mf_tile_kernel      the fp64 pair-tile walker of pair_tile.hpp (lane layout, staging and LDS documented there) for the
//                       Gram product B A^T: a workgroup owns 64 rows of B and walks a chunk of column tiles of A; every
//                       tile's d^2 goes through LDS to the epilogue:
//                         radii  each row keeps its smallest values (the diagonal skipped by index)
//                         cross  each row counts the columns whose sphere holds it and keeps its smallest d^2
//                       the N x M matrix is never written to memory
//   mf_merge_*_kernel   the chunks' partials of a row merged in chunk order, one thread per row
// No atomics.  g_ij has one summation order (features in order, no split over F); sums of integers, minima and "the k
// smallest" do not depend on how the columns are split: two runs and any two split plans give the same bits.
#include <math.h>

#include "pair_tile.hpp"

static bool mf_rows_ok(long n) { return n >= 1 && n <= MMVAE_MANIFOLD_MAX_ROWS; }
static bool mf_f_ok(int F) { return F >= 1 && F <= MMVAE_FRECHET_MAX_F; }
static bool mf_k_ok(int k) { return k >= 1 && k <= MMVAE_MANIFOLD_MAX_K; }

// -> column tiles per chunk and the chunks that hold at least one tile; `chunks` 0: the default plan
static void mf_plan(long rows, long cols, int chunks, int* tiles_per_chunk, int* n_chunks) {
  pair_plan(pt_tiles(rows), pt_tiles(cols), chunks, PT_SLOTS, PT_MIN_TILES, tiles_per_chunk, n_chunks);
}

// ---- squared norms -------------------------------------------------------------------------------------------------------
// grid ceil(rows / 64), 256 threads: 64 x 64 fp32 blocks of X go through LDS (coalesced loads); thread t < 64 owns row t and
// adds the squares in feature order
__global__ __launch_bounds__(256) void mf_sqnorms_kernel(const float* __restrict__ X, double* __restrict__ n2, long rows,
                                                         int F) {
  __shared__ float blk[64][65];
  const int tid = threadIdx.x, c = tid & 63, r4 = tid >> 6;
  const long i0 = (long)blockIdx.x * 64;
  double s = 0.0;
  for (int f0 = 0; f0 < F; f0 += 64) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = r4 + 4 * e;
      blk[r][c] = (i0 + r < rows && f0 + c < F) ? X[(size_t)(i0 + r) * F + f0 + c] : 0.0f;
    }
    __syncthreads();
    if (tid < 64) {
#pragma unroll 8
      for (int f = 0; f < 64; ++f) {
        const double v = (double)blk[tid][f];
        s += v * v;
      }
    }
  }
  if (tid < 64 && i0 + tid < rows) n2[i0 + tid] = s;
}

// ---- a sorted list of the KEEP smallest values, in registers ---------------------------------------------------------------
// (every index is a compile-time constant after unrolling; slots beyond the values met so far hold +inf)
template <int KEEP>
struct MfKeep {
  double v[KEEP];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < KEEP; ++s) v[s] = INFINITY;
  }
  __device__ __forceinline__ void put(double x) {
    if (!(x < v[KEEP - 1])) return;
#pragma unroll
    for (int s = 0; s < KEEP; ++s) {
      const double lo = fmin(v[s], x);
      x = fmax(v[s], x);
      v[s] = lo;
    }
  }
};

// ---- the tile kernel: the policies of pair_tile_walk ---------------------------------------------------------------------------
// rows i0 + r of B and j0 + r of A, addressed directly
struct MfRows {
  const float *Bm, *Am;
  long i0, rows_b, rows_a;
  int F;
  __device__ __forceinline__ void columns(long) {}
  __device__ __forceinline__ float b(int e, int k0) const {
    const int r = threadIdx.x / PT_KT + (256 / PT_KT) * e, kk = threadIdx.x % PT_KT;
    return (k0 + kk < F && i0 + r < rows_b) ? Bm[(size_t)(i0 + r) * F + k0 + kk] : 0.0f;
  }
  __device__ __forceinline__ float a(int e, long j0, int k0) const {
    const int r = threadIdx.x / PT_KT + (256 / PT_KT) * e, kk = threadIdx.x % PT_KT;
    return (k0 + kk < F && j0 + r < rows_a) ? Am[(size_t)(j0 + r) * F + k0 + kk] : 0.0f;
  }
};

// d^2 from the norms and the dot product, and what a row keeps of it:
// KEEP > 0, the radii (B == A, k <= KEEP): part (chunks, rows_b, k) = the k smallest d^2 of the chunk per row, ascending,
//   +inf where fewer were met.
// KEEP == 0, the cross pass: part (chunks, rows_b, 2) = (number of columns i with d^2 <= rad2_a[i], smallest d^2) of the
//   chunk per row; rad2_a of the tile's columns is staged in LDS with the d^2 tile (this instantiation's 512 bytes).
template <int KEEP>
struct MfEpilogue {
  static constexpr bool RADII = KEEP > 0;
  const double *nb, *na, *rad2_a;
  long i0, rows_b, rows_a;
  MfKeep<RADII ? KEEP : 1> keep;
  int count;
  double nearest;
  __device__ __forceinline__ static double* rad_s() {
    __shared__ double s[PT_TILE];
    return s;
  }
  __device__ __forceinline__ void stage(int t) {
    const long j = (long)t * PT_TILE + threadIdx.x;
    if constexpr (!RADII)
      if (threadIdx.x < PT_TILE) rad_s()[threadIdx.x] = j < rows_a ? rad2_a[j] : 0.0;
  }
  __device__ __forceinline__ double column(int t, int cj) const {
    const long j = (long)t * PT_TILE + cj;
    return j < rows_a ? na[j] : 0.0;
  }
  __device__ __forceinline__ double element(double ncol, int ci, double g) const {
    const double nrow = i0 + ci < rows_b ? nb[i0 + ci] : 0.0;
    return fmax(0.0, (nrow + ncol) - 2.0 * g);
  }
  __device__ __forceinline__ void tile(const double* lds, int t) {
    const int erow = threadIdx.x >> 2, equarter = threadIdx.x & 3;
    const long j0 = (long)t * PT_TILE, ei = i0 + erow;
    if (ei >= rows_b) return;
#pragma unroll 4
    for (int c = equarter; c < PT_TILE; c += 4) {
      const long j = j0 + c;
      if (j >= rows_a) break;
      const double d2 = lds[erow * PT_LDD + c];
      if constexpr (RADII) {
        if (j != ei) keep.put(d2);
      } else {
        count += d2 <= rad_s()[c] ? 1 : 0;
        nearest = fmin(nearest, d2);
      }
    }
  }
  // the four quarters of a row are four neighbouring lanes
  __device__ __forceinline__ void write(double* __restrict__ part, int k) {
    const int lane = threadIdx.x & 63, equarter = threadIdx.x & 3;
    const long ei = i0 + (threadIdx.x >> 2);
    double* out = part + ((size_t)blockIdx.x * rows_b + ei) * k;
    if constexpr (RADII) {
#pragma unroll
      for (int q = 1; q < 4; ++q)
#pragma unroll
        for (int s = 0; s < KEEP; ++s) {
          const double other = __shfl(keep.v[s], (lane & ~3) + q, 64);
          if (equarter == 0) keep.put(other);
        }
      if (equarter == 0 && ei < rows_b) {
#pragma unroll
        for (int s = 0; s < KEEP; ++s)
          if (s < k) out[s] = keep.v[s];
      }
    } else {
#pragma unroll
      for (int o = 1; o < 4; o <<= 1) {
        count += __shfl_xor(count, o, 64);
        nearest = fmin(nearest, __shfl_xor(nearest, o, 64));
      }
      if (equarter == 0 && ei < rows_b) {
        out[0] = (double)count;
        out[1] = nearest;
      }
    }
  }
};

// grid (chunks, row tiles), 256 threads.  Workgroup (c, t) owns the rows [64 t, 64 t + 64) of B against the column tiles
// [c tpc, (c + 1) tpc) of A; k = 2 for the cross pass.
template <int KEEP>
__global__ __launch_bounds__(256, 2) void mf_tile_kernel(const float* __restrict__ Bm, const double* __restrict__ nb,
                                                      const float* __restrict__ Am, const double* __restrict__ na,
                                                      const double* __restrict__ rad2_a, double* __restrict__ part,
                                                      long rows_b, long rows_a, int F, int k, int tpc) {
  const long i0 = (long)blockIdx.y * PT_TILE;
  const int t0 = blockIdx.x * tpc, t1 = min(pt_tiles(rows_a), t0 + tpc);
  MfEpilogue<KEEP> epi{nb, na, rad2_a, i0, rows_b, rows_a, {}, 0, INFINITY};
  epi.keep.clear();
  pair_tile_walk(MfRows{Bm, Am, i0, rows_b, rows_a, F}, epi, F, t0, t1);
  epi.write(part, k);
}

// ---- merges: one thread per row, the chunks in order -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void mf_merge_radii_kernel(const double* __restrict__ part, double* __restrict__ rad2,
                                                             long rows, int k, int chunks) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  MfKeep<MMVAE_MANIFOLD_MAX_K> keep;
  keep.clear();
  for (int c = 0; c < chunks; ++c) {
    const double* p = part + ((size_t)c * rows + i) * k;
    for (int s = 0; s < k; ++s) keep.put(p[s]);
  }
  double out = INFINITY;
#pragma unroll
  for (int s = 0; s < MMVAE_MANIFOLD_MAX_K; ++s)
    if (s == k - 1) out = keep.v[s];
  rad2[i] = out;
}

__global__ __launch_bounds__(256) void mf_merge_cross_kernel(const double* __restrict__ part, int* __restrict__ count,
                                                             double* __restrict__ mind2, long rows, int chunks) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  int n = 0;
  double nearest = INFINITY;
  for (int c = 0; c < chunks; ++c) {
    const double* p = part + ((size_t)c * rows + i) * 2;
    n += (int)p[0];
    nearest = fmin(nearest, p[1]);
  }
  count[i] = n;
  mind2[i] = nearest;
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" int mmvae_manifold_chunks(long rows, long cols) {
  if (!mf_rows_ok(rows) || !mf_rows_ok(cols)) return 0;
  int tpc, n;
  mf_plan(rows, cols, 0, &tpc, &n);
  return n;
}

extern "C" size_t mmvae_manifold_ws_doubles(long rows, long cols, int k, int chunks) {
  if (!mf_rows_ok(rows) || !mf_rows_ok(cols) || !mf_k_ok(k) || chunks < 0) return 0;
  int tpc, n;
  mf_plan(rows, cols, chunks, &tpc, &n);
  return (size_t)n * (size_t)rows * (size_t)(k < 2 ? 2 : k);
}

extern "C" int mmvae_manifold_sqnorms(const float* X, double* n2, long rows, int F, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && n2);
  if (!mf_rows_ok(rows) || !mf_f_ok(F)) return MMVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mf_sqnorms_kernel, dim3(pt_tiles(rows)), dim3(256), 0, (hipStream_t)stream, X, n2, rows, F);
  return mmvae_launch_status();
}

extern "C" int mmvae_manifold_radii(const float* X, const double* n2, double* ws, double* rad2, long rows, int F, int k,
                                    int chunks, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && n2 && ws && rad2);
  if (!mf_rows_ok(rows) || !mf_f_ok(F) || !mf_k_ok(k) || rows < (long)k + 1 || chunks < 0) return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int tpc, n;
  mf_plan(rows, rows, chunks, &tpc, &n);
  const dim3 grid(n, pt_tiles(rows));
  const double* none = nullptr;
  // the registers of a row's lists follow k: 4, 8 or MMVAE_MANIFOLD_MAX_K slots per epilogue thread
  if (k <= 4)
    hipLaunchKernelGGL((mf_tile_kernel<4>), grid, dim3(256), 0, s, X, n2, X, n2, none, ws, rows, rows, F, k, tpc);
  else if (k <= 8)
    hipLaunchKernelGGL((mf_tile_kernel<8>), grid, dim3(256), 0, s, X, n2, X, n2, none, ws, rows, rows, F, k, tpc);
  else
    hipLaunchKernelGGL((mf_tile_kernel<MMVAE_MANIFOLD_MAX_K>), grid, dim3(256), 0, s, X, n2, X, n2, none, ws, rows, rows, F,
                       k, tpc);
  hipLaunchKernelGGL(mf_merge_radii_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, ws, rad2, rows, k, n);
  return mmvae_launch_status();
}

extern "C" int mmvae_manifold_cross(const float* B, const double* nb, const float* A, const double* na,
                                    const double* rad2_a, double* ws, int* count, double* mind2, long rows_b, long rows_a,
                                    int F, int chunks, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(B && nb && A && na && rad2_a && ws && count && mind2);
  if (!mf_rows_ok(rows_b) || !mf_rows_ok(rows_a) || !mf_f_ok(F) || chunks < 0) return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int tpc, n;
  mf_plan(rows_b, rows_a, chunks, &tpc, &n);
  hipLaunchKernelGGL((mf_tile_kernel<0>), dim3(n, pt_tiles(rows_b)), dim3(256), 0, s, B, nb, A, na, rad2_a, ws, rows_b,
                     rows_a, F, 2, tpc);
  hipLaunchKernelGGL(mf_merge_cross_kernel, dim3((unsigned)((rows_b + 255) / 256)), dim3(256), 0, s, ws, count, mind2, rows_b,
                     n);
  return mmvae_launch_status();
}
