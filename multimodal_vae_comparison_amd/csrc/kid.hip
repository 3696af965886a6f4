// Kernel inception distance of generated images (TorchMMVAE.kernel_distances; Binkowski et al. 2018): the unbiased MMD^2
// between real and generated features under the polynomial kernel k(x, y) = (gamma x . y + coef0)^degree, over S random
// subsets of m rows each.  Per subset s and pair, with x_i = X[idx_x[s, i]] and y_j = Y[idx_y[s, j]]:
//   sxx = sum_{i != j} k(x_i, x_j)   syy = sum_{i != j} k(y_i, y_j)   (the diagonal left out by POSITION i == j)
//   sxy = sum_{i, j} k(x_i, y_j)                                       (all m^2 terms)
//   kid_tile_kernel   the fp64 pair-tile walker of pair_tile.hpp (lane layout, staging and LDS documented there) with two
//                     policies of its own: the rows of a tile are ADDRESSED THROUGH THE INDEX LIST in the fetch (fp32
//                     converted to double on load; no gathered copy of the rows exists), and the epilogue applies the kernel
//                     function to the tile's dot products and SUMS them per row.  One launch covers every (subset, pair)
//                     slice.  The two within-set pairs are symmetric: only the column tiles on or above the diagonal tile are
//                     walked, the tiles strictly above it counted twice (a product by 2 is exact).  The m x m block is never
//                     written.
//   kid_sum_kernel    the row partials of a slice added in a fixed order, one workgroup per slice
// No atomics.  g_ij has one summation order (features in order, no split over F).  For a given (m, chunks) two runs give the
// same bits; two chunk plans regroup fp64 sums and agree to rounding only.
#include "pair_tile.hpp"

static bool kd_shape_ok(int subsets, long m) {
  return subsets >= 1 && subsets <= MMVAE_KID_MAX_SUBSETS && m >= 2 && m <= MMVAE_KID_MAX_SUBSET;
}

// -> column tiles per chunk and the chunks that hold at least one tile; `chunks` 0: the default plan
static void kd_plan(int subsets, long m, int chunks, int* tiles_per_chunk, int* n_chunks) {
  const int ct = pt_tiles(m);
  pair_plan(3L * subsets * ct, ct, chunks, PT_SLOTS, PT_MIN_TILES, tiles_per_chunk, n_chunks);
}

// ---- the tile kernel: the policies of pair_tile_walk ---------------------------------------------------------------------------
// the rows ib[i0 + r] of B and ia[j0 + r] of A: a thread keeps the eight row numbers of both lists that it stages in
// registers (-1 past the end of the list: zeros are staged); the next tile's are read before its first fetch
struct KidRows {
  const float *Bm, *Am;
  const int *ib, *ia;
  long m;
  int F;
  int rb[PT_LOADS], ra[PT_LOADS];      // (not initialised: rows_of fills them before the first fetch)
  __device__ __forceinline__ KidRows(const float* Bm, const float* Am, const int* ib, const int* ia, long m, int F)
      : Bm(Bm), Am(Am), ib(ib), ia(ia), m(m), F(F) {}
  __device__ __forceinline__ void rows_of(const int* list, long p0, int (&rows)[PT_LOADS]) const {
    const int frow = threadIdx.x / PT_KT;
#pragma unroll
    for (int e = 0; e < PT_LOADS; ++e) {
      const long p = p0 + frow + (256 / PT_KT) * e;
      rows[e] = p < m ? list[p] : -1;
    }
  }
  __device__ __forceinline__ void columns(long j0) { rows_of(ia, j0, ra); }
  __device__ __forceinline__ float b(int e, int k0) const {
    const int kk = threadIdx.x % PT_KT;
    return (k0 + kk < F && rb[e] >= 0) ? Bm[(size_t)rb[e] * F + k0 + kk] : 0.0f;
  }
  __device__ __forceinline__ float a(int e, long, int k0) const {
    const int kk = threadIdx.x % PT_KT;
    return (k0 + kk < F && ra[e] >= 0) ? Am[(size_t)ra[e] * F + k0 + kk] : 0.0f;
  }
};

// the kernel function of a dot product; a position's sum over the columns walked, the diagonal of a symmetric pair left
// out by position and its tiles strictly above the diagonal tile counted twice
struct KidEpilogue {
  int degree;
  double gamma, coef0;
  long i0, m;
  bool symmetric;
  double rowsum;
  __device__ __forceinline__ void stage(int) {}
  __device__ __forceinline__ double column(int, int) const { return 0.0; }      // (the kernel function has no column term)
  __device__ __forceinline__ double element(double, int, double g) const {
    const double base = gamma * g + coef0;
    double v = base;
    for (int q = 1; q < degree; ++q) v *= base;
    return v;
  }
  __device__ __forceinline__ void tile(const double* lds, int t) {
    const int erow = threadIdx.x >> 2, equarter = threadIdx.x & 3;
    const long j0 = (long)t * PT_TILE, ei = i0 + erow;
    if (ei < m) {
      double tile = 0.0;
#pragma unroll 4
      for (int c = equarter; c < PT_TILE; c += 4) {
        const long j = j0 + c;
        if (j >= m) break;
        if (!symmetric || j != ei) tile += lds[erow * PT_LDD + c];
      }
      rowsum += (symmetric && t > (int)blockIdx.y) ? 2.0 * tile : tile;
    }
  }
};

// grid (chunks, row tiles, 3 S), 256 threads.  Slice z = 3 s + pair, pair 0: xx, 1: yy, 2: xy.  Workgroup (c, t, z) owns the
// positions [64 t, 64 t + 64) of the slice's row list against the column tiles [c tpc, (c + 1) tpc) of its column list
// (xx, yy: from tile t on).  part (3 S, chunks, m): the sum of a position's kernel values over the chunk's columns (0 where
// the chunk holds no tile of the row tile).
__global__ __launch_bounds__(256, 2) void kid_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                       const int* __restrict__ idx_x, const int* __restrict__ idx_y,
                                                       double* __restrict__ part, int F, long m, int degree, double gamma,
                                                       double coef0, int tpc) {
  const int slice = blockIdx.z, s = slice / 3, pair = slice - 3 * s;
  const bool symmetric = pair < 2;
  const long i0 = (long)blockIdx.y * PT_TILE;
  int t0 = blockIdx.x * tpc;
  const int t1 = min(pt_tiles(m), t0 + tpc);
  if (symmetric) t0 = max(t0, (int)blockIdx.y);
  KidRows rows(pair == 1 ? Y : X, pair == 0 ? X : Y, (pair == 1 ? idx_y : idx_x) + (size_t)s * m,
               (pair == 0 ? idx_x : idx_y) + (size_t)s * m, m, F);
  KidEpilogue epi{degree, gamma, coef0, i0, m, symmetric, 0.0};
  if (t0 < t1) rows.rows_of(rows.ib, i0, rows.rb);
  pair_tile_walk(rows, epi, F, t0, t1);
  // the four quarters of a row are four neighbouring lanes
#pragma unroll
  for (int o = 1; o < 4; o <<= 1) epi.rowsum += __shfl_xor(epi.rowsum, o, 64);
  const long ei = i0 + (threadIdx.x >> 2);
  if ((threadIdx.x & 3) == 0 && ei < m) part[((size_t)slice * gridDim.x + blockIdx.x) * m + ei] = epi.rowsum;
}


// ---- the sum of a slice: grid 3 S, 256 threads -----------------------------------------------------------------------------------
// thread t adds the partials of the positions t, t + 256, ... (per position the chunks in order), then a tree over the 256
// threads in LDS: a fixed order
__global__ __launch_bounds__(256) void kid_sum_kernel(const double* __restrict__ part, double* __restrict__ sums, long m,
                                                      int chunks) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const double* p = part + (size_t)blockIdx.x * chunks * m;
  double s = 0.0;
  for (long i = tid; i < m; i += 256)
    for (int c = 0; c < chunks; ++c) s += p[(size_t)c * m + i];
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) sums[blockIdx.x] = red[0];
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" int mmvae_kid_chunks(int subsets, long m) {
  if (!kd_shape_ok(subsets, m)) return 0;
  int tpc, n;
  kd_plan(subsets, m, 0, &tpc, &n);
  return n;
}

extern "C" size_t mmvae_kid_ws_doubles(int subsets, long m, int chunks) {
  if (!kd_shape_ok(subsets, m) || chunks < 0) return 0;
  int tpc, n;
  kd_plan(subsets, m, chunks, &tpc, &n);
  return (size_t)3 * (size_t)subsets * (size_t)n * (size_t)m;
}

extern "C" int mmvae_kid_sums(const float* X, const float* Y, const int* idx_x, const int* idx_y, double* ws, double* sums,
                              long rows_x, long rows_y, int F, int subsets, long m, int degree, double gamma, double coef0,
                              int chunks, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && Y && idx_x && idx_y && ws && sums);
  if (!kd_shape_ok(subsets, m) || F < 1 || F > MMVAE_FRECHET_MAX_F || degree < 1 || degree > MMVAE_KID_MAX_DEGREE ||
      rows_x < 1 || rows_y < 1 || chunks < 0)
    return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int tpc, n;
  kd_plan(subsets, m, chunks, &tpc, &n);
  hipLaunchKernelGGL(kid_tile_kernel, dim3(n, pt_tiles(m), 3 * subsets), dim3(256), 0, s, X, Y, idx_x, idx_y, ws, F, m,
                     degree, gamma, coef0, tpc);
  hipLaunchKernelGGL(kid_sum_kernel, dim3(3 * subsets), dim3(256), 0, s, ws, sums, m, n);
  return mmvae_launch_status();
}
