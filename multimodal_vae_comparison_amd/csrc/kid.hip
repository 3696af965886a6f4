// Kernel inception distance of generated images (TorchMMVAE.kernel_distances; Binkowski et al. 2018): the unbiased MMD^2
// between real and generated features under the polynomial kernel k(x, y) = (gamma x . y + coef0)^degree, over S random
// subsets of m rows each.  Per subset s and pair, with x_i = X[idx_x[s, i]] and y_j = Y[idx_y[s, j]]:
//   sxx = sum_{i != j} k(x_i, x_j)   syy = sum_{i != j} k(y_i, y_j)   (the diagonal left out by POSITION i == j)
//   sxy = sum_{i, j} k(x_i, y_j)                                       (all m^2 terms)
//   kid_tile_kernel   the rectangular fp64 MFMA tile routine of manifold.hip (v_mfma_f64_16x16x4_f64; 64 x 64 tile per
//                     workgroup, 32 x 32 per wave; lane layout and staging as documented at mf_tile_kernel) with two new
//                     things: the rows of a tile are ADDRESSED THROUGH THE INDEX LIST in the fetch (fp32 converted to double
//                     on load; no gathered copy of the rows exists), and the epilogue applies the kernel function to the
//                     tile's dot products and SUMS them per row.  One launch covers every (subset, pair) slice.  The two
//                     within-set pairs are symmetric: only the column tiles on or above the diagonal tile are walked, the
//                     tiles strictly above it counted twice (a product by 2 is exact).  The m x m block is never written.
//   kid_sum_kernel    the row partials of a slice added in a fixed order, one workgroup per slice
// No atomics.  g_ij has one summation order (features in order, no split over F).  For a given (m, chunks) two runs give the
// same bits; two chunk plans regroup fp64 sums and agree to rounding only.
#include "common.hpp"

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define KD_TILE 64                 // tile of a workgroup: positions of the row list x positions of the column list
#define KD_KT 32                   // feature depth of a staged tile
#define KD_LDS (KD_TILE + 2)       // LDS row stride of a staged operand, in doubles
#define KD_LDD (KD_TILE + 4)       // LDS row stride of the tile of kernel values (as manifold.hip's d^2 tile)
#define KD_LOADS (KD_TILE * KD_KT / 256)      // elements of each operand a thread stages per step
#define KD_SLOTS 512               // workgroups wanted in flight: 256 CUs x 2 (34.8 KB of LDS each)
#define KD_MIN_TILES 4             // column tiles per chunk at least

static bool kd_shape_ok(int subsets, long m) {
  return subsets >= 1 && subsets <= MMVAE_KID_MAX_SUBSETS && m >= 2 && m <= MMVAE_KID_MAX_SUBSET;
}
static int kd_tiles(long m) { return (int)((m + KD_TILE - 1) / KD_TILE); }

// -> column tiles per chunk and the chunks that hold at least one tile; `chunks` 0: the default plan
static void kd_plan(int subsets, long m, int chunks, int* tiles_per_chunk, int* n_chunks) {
  const int ct = kd_tiles(m);
  if (chunks <= 0) {
    const long groups = 3L * subsets * ct;      // workgroups of an unsplit launch
    chunks = (int)((KD_SLOTS + groups - 1) / groups);
    const int most = (ct + KD_MIN_TILES - 1) / KD_MIN_TILES;
    if (chunks > most) chunks = most;
  }
  if (chunks > ct) chunks = ct;
  *tiles_per_chunk = (ct + chunks - 1) / chunks;
  *n_chunks = (ct + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

// ---- the tile routine ---------------------------------------------------------------------------------------------------------
// grid (chunks, row tiles, 3 S), 256 threads.  Slice z = 3 s + pair, pair 0: xx, 1: yy, 2: xy.  Workgroup (c, t, z) owns the
// positions [64 t, 64 t + 64) of the slice's row list against the column tiles [c tpc, (c + 1) tpc) of its column list
// (xx, yy: from tile t on).  A thread stages the features k0 + tid % 32 of the rows tid / 32 + 8 e, e < 8, of each operand:
// it keeps those eight row numbers of both lists in registers (-1 past the end of the list: zeros are staged) and the
// next tile's are read before its first fetch.  Epilogue thread e = 4 row + quarter reads the columns quarter, quarter + 4,
// ... of its row.  part (3 S, chunks, m): the sum of a position's kernel values over the chunk's columns (0 where the
// chunk holds no tile of the row tile).
__global__ __launch_bounds__(256, 2) void kid_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                       const int* __restrict__ idx_x, const int* __restrict__ idx_y,
                                                       double* __restrict__ part, int F, long m, int degree, double gamma,
                                                       double coef0, int tpc) {
  __shared__ double lds[KD_TILE * KD_LDD];      // the tile of kernel values; the staged operands live in its first 2 KD_KT
                                                // KD_LDS doubles
  double(*Bs)[KD_LDS] = reinterpret_cast<double(*)[KD_LDS]>(lds);
  double(*As)[KD_LDS] = reinterpret_cast<double(*)[KD_LDS]>(lds + KD_KT * KD_LDS);
  static_assert(2 * KD_KT * KD_LDS <= KD_TILE * KD_LDD, "the staged operands fit inside the tile of kernel values");
  const int slice = blockIdx.z, s = slice / 3, pair = slice - 3 * s;
  const bool symmetric = pair < 2;
  const float* __restrict__ Bm = pair == 1 ? Y : X;
  const float* __restrict__ Am = pair == 0 ? X : Y;
  const int* __restrict__ ib = (pair == 1 ? idx_y : idx_x) + (size_t)s * m;
  const int* __restrict__ ia = (pair == 0 ? idx_x : idx_y) + (size_t)s * m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long i0 = (long)blockIdx.y * KD_TILE;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, lr = lane & 15, lk = lane >> 4;
  const int erow = tid >> 2, equarter = tid & 3;
  const long ei = i0 + erow;
  const int frow = tid / KD_KT, fk = tid % KD_KT;      // element e of a thread: row frow + 8 e of the tile, feature fk
  const int ct = (int)((m + KD_TILE - 1) / KD_TILE);
  int t0 = blockIdx.x * tpc;
  const int t1 = min(ct, t0 + tpc);
  if (symmetric) t0 = max(t0, (int)blockIdx.y);
  double rowsum = 0.0;
  int rb[KD_LOADS], ra[KD_LOADS];
  float pb[KD_LOADS], pa[KD_LOADS];
  auto rows_of = [&](const int* __restrict__ list, long p0, int* rows) {
#pragma unroll
    for (int e = 0; e < KD_LOADS; ++e) {
      const long p = p0 + frow + (256 / KD_KT) * e;
      rows[e] = p < m ? list[p] : -1;
    }
  };
  auto fetch = [&](int k0) {
    const bool kin = k0 + fk < F;
#pragma unroll
    for (int e = 0; e < KD_LOADS; ++e) {
      pb[e] = (kin && rb[e] >= 0) ? Bm[(size_t)rb[e] * F + k0 + fk] : 0.0f;
      pa[e] = (kin && ra[e] >= 0) ? Am[(size_t)ra[e] * F + k0 + fk] : 0.0f;
    }
  };
  if (t0 < t1) {
    rows_of(ib, i0, rb);
    rows_of(ia, (long)t0 * KD_TILE, ra);
    fetch(0);
  }
  for (int t = t0; t < t1; ++t) {
    const long j0 = (long)t * KD_TILE;
    f64x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < F; k0 += KD_KT) {
      __syncthreads();      // (the previous tile's epilogue, or the previous step's MFMAs, have read the LDS)
#pragma unroll
      for (int e = 0; e < KD_LOADS; ++e) {
        const int r = frow + (256 / KD_KT) * e;
        Bs[fk][r] = (double)pb[e];
        As[fk][r] = (double)pa[e];
      }
      __syncthreads();
      if (k0 + KD_KT < F) {
        fetch(k0 + KD_KT);
      } else if (t + 1 < t1) {
        rows_of(ia, j0 + KD_TILE, ra);
        fetch(0);
      }
#pragma unroll 2
      for (int k4 = 0; k4 < KD_KT; k4 += 4) {
        double bv[2], av[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          bv[u] = Bs[k4 + lk][wm + 16 * u + lr];
          av[u] = As[k4 + lk][wn + 16 * u + lr];
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[mi], av[ni], acc[mi][ni], 0, 0, 0);
      }
    }
    __syncthreads();        // (the last MFMAs have read the staged operands the tile overwrites)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int cj = wn + 16 * ni + lr;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ci = wm + 16 * mi + lk + 4 * r;
          const double base = gamma * acc[mi][ni][r] + coef0;
          double v = base;
          for (int q = 1; q < degree; ++q) v *= base;
          lds[ci * KD_LDD + cj] = v;
        }
    }
    __syncthreads();
    if (ei < m) {
      double tile = 0.0;
#pragma unroll 4
      for (int c = equarter; c < KD_TILE; c += 4) {
        const long j = j0 + c;
        if (j >= m) break;
        if (!symmetric || j != ei) tile += lds[erow * KD_LDD + c];
      }
      rowsum += (symmetric && t > (int)blockIdx.y) ? 2.0 * tile : tile;
    }
  }
  // the four quarters of a row are four neighbouring lanes
#pragma unroll
  for (int o = 1; o < 4; o <<= 1) rowsum += __shfl_xor(rowsum, o, 64);
  if (equarter == 0 && ei < m) part[((size_t)slice * gridDim.x + blockIdx.x) * m + ei] = rowsum;
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
  hipLaunchKernelGGL(kid_tile_kernel, dim3(n, kd_tiles(m), 3 * subsets), dim3(256), 0, s, X, Y, idx_x, idx_y, ws, F, m,
                     degree, gamma, coef0, tpc);
  hipLaunchKernelGGL(kid_sum_kernel, dim3(3 * subsets), dim3(256), 0, s, ws, sums, m, n);
  return mmvae_launch_status();
}
