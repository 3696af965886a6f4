// Kernel two-sample test of latents (TorchMMVAE.latent_two_sample; Gretton et al. 2012): the sums behind the unbiased MMD^2
// of two sets of rows X (n_x, D), Y (n_y, D), for the observed split and for P relabellings of the pooled sample (X's rows,
// then Y's; n = n_x + n_y), under a characteristic kernel of the squared distance d^2 = |x - y|^2:
//   rbf     k = (1 / S) sum_s exp(-gamma_s d^2)        imq     k = (1 / S) sum_s c_s / (c_s + d^2)        energy  k = -d
// Per split with indicator a (1: the row counts as "X"), K the n x n kernel matrix with its diagonal left out by POSITION:
//   r = K 1 (row_sums)   T = 1' r   sxx = a' K a   sxy = (1 - a)' K a   syy = (T - sxx) - 2 sxy
// so a split needs one all-pairs product K a, and that is a product of Gram tiles with a block of 0/1 columns.  sxx and
// sxy are sums of their own terms only (nothing is lost when one of them is small beside T).
//   mmd_mean_kernel     the pooled mean per feature, in double, a fixed order (and the kernel parameters into the workspace)
//   mmd_centre_kernel   Z = row - mean in double (n, D): the three families are translation invariant, and on centred rows
//                       the Gram form |x|^2 + |y|^2 - 2 x . y loses nothing to an offset of the data
//   mmd_pack_kernel     the indicator columns (0: the observed split, 1 + p: relabelling p; zeros up to a multiple of
//                       MMVAE_MMD_PBLOCK) as bytes in the order a lane of the product reads them
//   mmd_norm_kernel     |z_i|^2 as the DIAGONAL of the walker's own Gram tile: the bits of z_i . z_j for a row j equal to
//                       row i, so duplicate rows give (n + n) - 2 n = 0 in the Gram form
//   mmd_tile_kernel     the fp64 pair-tile walker of pair_tile.hpp (lane layout, staging and LDS documented there) with a
//                       Rows policy that reads the centred doubles and an Epilogue that turns the tile into d^2 (pairs that
//                       the Gram form resolves badly again by differences: MMD_CLOSE), applies the kernel function
//                       (0 on the diagonal and outside the sample) and multiplies the 64 x 64 tile in LDS by the
//                       64 x MMVAE_MMD_PBLOCK block of indicators of its columns on v_mfma_f64_16x16x4_f64; the product is
//                       dotted with the indicators of the row tile at once and added to the lane's sum over the chunk's
//                       column tiles.  The first block of columns also adds the rows of every tile (the row sums).  The
//                       n x n matrix is never written.
//   mmd_rows_kernel     r_i: the chunks' partials of a row in chunk order
//   mmd_sums_kernel     per split T, sxx and sxy, each in one fixed order, and syy
// No atomics.  Two runs with one plan give the same bits; a split's sums do not depend on which column it occupies or on
// what the other columns hold; two chunk plans regroup fp64 sums and agree to rounding only.
#include <math.h>

#include "pair_tile.hpp"

#define MMD_PB MMVAE_MMD_PBLOCK      // indicator columns of a workgroup: 32 per wave, 64 product registers per lane
#define MMD_EXTRA 1                  // column 0: the observed split
// The Gram form's error in d^2 is a few roundings of |z_i|^2 + |z_j|^2, whatever d^2 is: a pair whose d^2 comes out below
// this share of that sum (close rows of a wide sample: two clusters far apart, say) is computed again by differences,
// features in order -- as exact as the rows themselves, and exactly 0 for rows with equal bits.
#define MMD_CLOSE 0.25

static bool md_shape_ok(long n, int D, int P) {
  return n >= 4 && n <= MMVAE_MMD_MAX_ROWS && D >= 1 && D <= MMVAE_MMD_MAX_D && P >= 0 && P <= MMVAE_MMD_MAX_PERMUTATIONS;
}
static int md_columns(int P) { return (P + MMD_EXTRA + MMD_PB - 1) / MMD_PB * MMD_PB; }
static size_t md_even(size_t v) { return (v + 1) & ~(size_t)1; }

// -> column tiles per chunk and the chunks that hold at least one tile; `chunks` 0: the default plan, a function of n alone
// (a relabelling run alone and inside a batch must share it)
static void md_plan(long n, int chunks, int* tiles_per_chunk, int* n_chunks) {
  const int ct = pt_tiles(n);
  pair_plan(ct, ct, chunks, PT_SLOTS, PT_MIN_TILES, tiles_per_chunk, n_chunks);
}

// the workspace, in doubles (every part starts at an even offset: the packed indicators are read 16 bytes at a time)
struct MdWs {
  size_t prm, mean, n2, z, rowpart, part, packed, total;
};
static MdWs md_ws(long n, int D, int P, int n_chunks) {
  const size_t rt = (size_t)pt_tiles(n), pc = (size_t)md_columns(P);
  MdWs w;
  w.prm = 0;
  w.mean = w.prm + MMVAE_MMD_MAX_SCALES;
  w.n2 = w.mean + md_even((size_t)D);
  w.z = w.n2 + md_even((size_t)n);
  w.rowpart = w.z + md_even((size_t)n * (size_t)D);
  w.part = w.rowpart + md_even((size_t)n_chunks * (size_t)n);
  w.packed = w.part + 2 * rt * (size_t)n_chunks * pc;
  w.total = w.packed + rt * pc * (PT_TILE / 8);
  return w;
}

struct MdParams {
  double p[MMVAE_MMD_MAX_SCALES];
};

__device__ __forceinline__ float md_pooled(const float* __restrict__ X, const float* __restrict__ Y, long n_x, long i, int D,
                                           int d) {
  return i < n_x ? X[(size_t)i * D + d] : Y[(size_t)(i - n_x) * D + d];
}

// sum over the 256 threads of a workgroup, a fixed tree; the result in every thread
__device__ __forceinline__ double md_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// ---- the pooled mean: grid D, 256 threads ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mmd_mean_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                       double* __restrict__ mean, double* __restrict__ prm_out, MdParams prm,
                                                       long n_x, long n, int D) {
  __shared__ double red[256];
  const int d = blockIdx.x;
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += (double)md_pooled(X, Y, n_x, i, D, d);
  s = md_block_sum(s, red);
  if (threadIdx.x == 0) {
    mean[d] = s / (double)n;
    if (d == 0) {
#pragma unroll
      for (int k = 0; k < MMVAE_MMD_MAX_SCALES; ++k) prm_out[k] = prm.p[k];
    }
  }
}

// ---- the centred rows: one thread per element ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mmd_centre_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                         const double* __restrict__ mean, double* __restrict__ Z, long n_x,
                                                         long n, int D) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * D) return;
  const long i = (long)(e / D);
  const int d = (int)(e - (size_t)i * D);
  Z[e] = (double)md_pooled(X, Y, n_x, i, D, d) - mean[d];
}

// ---- the indicator columns as the product reads them -----------------------------------------------------------------------------
// packed (row tiles, pc, 4, 16) bytes: [t][c][lk][k4] = indicator c of the pooled row 64 t + 4 k4 + lk (0 past the sample and
// past the last column): the 16 bytes a lane (lk = lane >> 4) feeds to the 16 MFMAs of a tile.  One thread per 16 bytes.
__global__ __launch_bounds__(256) void mmd_pack_kernel(const unsigned char* __restrict__ member, uint4* __restrict__ packed,
                                                       long n_x, long n, int P, int pc) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t groups = (size_t)pt_tiles(n) * pc * 4;
  if (g >= groups) return;
  const int lk = (int)(g & 3);
  const int c = (int)((g >> 2) % pc);
  const long t = (long)((g >> 2) / pc);
  unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k4 = 0; k4 < 16; ++k4) {
    const long j = t * PT_TILE + 4 * k4 + lk;
    unsigned int bit = 0u;
    if (j < n && c < P + MMD_EXTRA)
      bit = c == 0 ? (j < n_x ? 1u : 0u) : (member[(size_t)(c - MMD_EXTRA) * n + j] ? 1u : 0u);
    w[k4 >> 2] |= bit << (8 * (k4 & 3));
  }
  packed[g] = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- the policies of pair_tile_walk ----------------------------------------------------------------------------------------------
// the centred rows i0 + r and j0 + r, doubles, addressed directly
struct MmdRows {
  const double* Z;
  long i0, n;
  int F;
  __device__ __forceinline__ void columns(long) {}
  __device__ __forceinline__ double b(int e, int k0) const {
    const int r = threadIdx.x / PT_KT + (256 / PT_KT) * e, kk = threadIdx.x % PT_KT;
    return (k0 + kk < F && i0 + r < n) ? Z[(size_t)(i0 + r) * F + k0 + kk] : 0.0;
  }
  __device__ __forceinline__ double a(int e, long j0, int k0) const {
    const int r = threadIdx.x / PT_KT + (256 / PT_KT) * e, kk = threadIdx.x % PT_KT;
    return (k0 + kk < F && j0 + r < n) ? Z[(size_t)(j0 + r) * F + k0 + kk] : 0.0;
  }
};

// the diagonal of the row tile's own Gram tile
struct MmdNormEpilogue {
  double* n2;
  long i0, n;
  __device__ __forceinline__ void stage(int) {}
  __device__ __forceinline__ double column(int, int) const { return 0.0; }
  __device__ __forceinline__ double element(double, int, double g) const { return g; }
  __device__ __forceinline__ void tile(const double* lds, int) {
    const int erow = threadIdx.x >> 2;
    if ((threadIdx.x & 3) == 0 && i0 + erow < n) n2[i0 + erow] = lds[erow * PT_LDD + erow];
  }
};

// grid row tiles, 256 threads
__global__ __launch_bounds__(256, 2) void mmd_norm_kernel(const double* __restrict__ Z, double* __restrict__ n2, long n,
                                                          int F) {
  const long i0 = (long)blockIdx.x * PT_TILE;
  MmdNormEpilogue epi{n2, i0, n};
  pair_tile_walk(MmdRows{Z, i0, n, F}, epi, F, (int)blockIdx.x, (int)blockIdx.x + 1);
}

template <int FAMILY>
__device__ __forceinline__ double mmd_kernel_value(double d2, const double* __restrict__ prm, int S) {
  if constexpr (FAMILY == MMVAE_MMD_ENERGY) {
    return -sqrt(d2);
  } else {
    double s = 0.0;
#pragma nounroll
    for (int k = 0; k < S; ++k) {
      const double p = prm[k];
      s += FAMILY == MMVAE_MMD_RBF ? exp(-p * d2) : p / (p + d2);
    }
    return s / (double)S;
  }
}

struct MmdColumn {
  double n2;
  long j;
};

// k(d^2) of the tile, then M = tile x indicators: wave w owns the columns [32 w, 32 w + 32) of the block against all 64
// rows, m[mi][ni] the 16 x 16 block at (rows 16 mi, columns 32 w + 16 ni); the lane holds M[16 mi + lk + 4 r][.. + lr] and
// adds its rows' share of a' M to qx[ni] and of (1 - a)' M to qc[ni] at once (rind: the row tile's own indicators, row
// 16 mi + lk + 4 r is byte 4 mi + r), so no accumulator block lives through the Gram product and the kernel function.  In the first block of
// columns thread e = 4 row + quarter also adds the tile's values of its row (the row sums).
template <int FAMILY>
struct MmdEpilogue {
  const double *Z, *n2, *prm;
  const unsigned char* packed;      // the block's first column of tile 0
  long i0, n;
  int F, S, pc;
  bool rows;
  uint4 rind[2];
  double qx[2], qc[2], rowsum;
  __device__ __forceinline__ const uint4* bytes(int t, int ni) const {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return reinterpret_cast<const uint4*>(packed + ((size_t)t * pc + 32 * wave + 16 * ni + (lane & 15)) * PT_TILE +
                                          16 * (lane >> 4));
  }
  __device__ __forceinline__ void stage(int) {}
  __device__ __forceinline__ MmdColumn column(int t, int cj) const {
    const long j = (long)t * PT_TILE + cj;
    return MmdColumn{j < n ? n2[j] : 0.0, j};
  }
  __device__ __forceinline__ double element(const MmdColumn& col, int ci, double g) const {
    const long i = i0 + ci;
    if (i >= n || col.j >= n || col.j == i) return 0.0;
    const double nn = n2[i] + col.n2;
    double d2 = fmax(0.0, nn - 2.0 * g);
    if (d2 < MMD_CLOSE * nn) {      // the Gram form has cancelled two bits or more: the pair again, by differences
      const double *zi = Z + (size_t)i * F, *zj = Z + (size_t)col.j * F;
      d2 = 0.0;
      for (int f = 0; f < F; ++f) {
        const double diff = zi[f] - zj[f];
        d2 = fma(diff, diff, d2);
      }
    }
    return mmd_kernel_value<FAMILY>(d2, prm, S);
  }
  __device__ __forceinline__ static double byte_of(const uint4& v, int k4) {
    const unsigned int w = k4 < 4 ? v.x : k4 < 8 ? v.y : k4 < 12 ? v.z : v.w;
    return (double)((w >> (8 * (k4 & 3))) & 0xffu);
  }
  __device__ __forceinline__ void tile(const double* lds, int t) {
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    uint4 ind[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) ind[ni] = *bytes(t, ni);
    if (rows) {      // (workgroup-uniform; values outside the sample and on the diagonal are zeros)
      const int erow = threadIdx.x >> 2, equarter = threadIdx.x & 3;
      double s = 0.0;
#pragma unroll 4
      for (int c = equarter; c < PT_TILE; c += 4) s += lds[erow * PT_LDD + c];
      rowsum += s;
    }
    f64x4 m[4][2] = {};
#pragma unroll
    for (int k4 = 0; k4 < PT_TILE / 4; ++k4) {
      double kv[4], bv[2];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) kv[mi] = lds[(16 * mi + lr) * PT_LDD + 4 * k4 + lk];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) bv[ni] = byte_of(ind[ni], k4);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) m[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[mi], bv[ni], m[mi][ni], 0, 0, 0);
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      // (opaque to the optimiser: it would otherwise keep the 32 bytes as 32 doubles, 64 registers, through the whole walk)
      uint4 ri = rind[ni];
      asm volatile("" : "+v"(ri.x), "+v"(ri.y), "+v"(ri.z), "+v"(ri.w));
      double sx = 0.0, sc = 0.0;      // (a row outside the sample has a zero row of the tile: it adds nothing to sc)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double a = byte_of(ri, 4 * mi + r);
          sx += a * m[mi][ni][r];
          sc += (1.0 - a) * m[mi][ni][r];
        }
      qx[ni] += sx;
      qc[ni] += sc;
    }
  }
};

// grid (chunks, row tiles, column blocks), 256 threads.  Workgroup (c, t, z) owns the rows [64 t, 64 t + 64) against the
// column tiles [c tpc, (c + 1) tpc) and the indicator columns [z PB, (z + 1) PB).
//   part (row tiles, chunks, pc, 2): sum_i a_i (K a)_i and sum_i (1 - a_i) (K a)_i over the workgroup's rows and the
//     chunk's columns: the terms of sxx and of sxy, each added up on its own
//   rowpart (chunks, n): (K 1)_i over the chunk's columns (written by the first block of columns)
template <int FAMILY>
__global__ __launch_bounds__(256, 2) void mmd_tile_kernel(const double* __restrict__ Z, const double* __restrict__ n2,
                                                          const double* __restrict__ prm,
                                                          const unsigned char* __restrict__ packed,
                                                          double* __restrict__ part, double* __restrict__ rowpart, long n,
                                                          int F, int S, int pc, int tpc) {
  const long i0 = (long)blockIdx.y * PT_TILE;
  const int t0 = blockIdx.x * tpc, t1 = min(pt_tiles(n), t0 + tpc);
  const int c0 = blockIdx.z * MMD_PB;
  MmdEpilogue<FAMILY> epi{Z, n2, prm, packed + (size_t)c0 * PT_TILE, i0, n, F, S, pc, blockIdx.z == 0, {}, {0.0, 0.0}, {0.0, 0.0}, 0.0};
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) epi.rind[ni] = *epi.bytes((int)blockIdx.y, ni);
  pair_tile_walk(MmdRows{Z, i0, n, F}, epi, F, t0, t1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    double qx = epi.qx[ni], qc = epi.qc[ni];      // the four row groups of a column are the lanes lr + 16 lk
    qx += __shfl_xor(qx, 16, 64);
    qx += __shfl_xor(qx, 32, 64);
    qc += __shfl_xor(qc, 16, 64);
    qc += __shfl_xor(qc, 32, 64);
    if (lk == 0) {
      double* out = part + 2 * (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * pc + c0 + 32 * wave + 16 * ni + lr);
      out[0] = qx;
      out[1] = qc;
    }
  }
  if (epi.rows) {      // the four quarters of a row are four neighbouring lanes
    double s = epi.rowsum;
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) s += __shfl_xor(s, o, 64);
    const long ei = i0 + (threadIdx.x >> 2);
    if ((threadIdx.x & 3) == 0 && ei < n) rowpart[(size_t)blockIdx.x * n + ei] = s;
  }
}

// ---- merges -------------------------------------------------------------------------------------------------------------------------
// one thread per row, the chunks in order
__global__ __launch_bounds__(256) void mmd_rows_kernel(const double* __restrict__ rowpart, double* __restrict__ row_sums,
                                                       long n, int chunks) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += rowpart[(size_t)c * n + i];
  row_sums[i] = s;
}

// grid 1 + P, 256 threads: workgroup b is the split of column b.  Thread t adds the terms t, t + 256, ... in order, then a
// tree over the 256 threads: T over the rows, sxx and sxy over (row tile, chunk); syy is what is left of T.
__global__ __launch_bounds__(256) void mmd_sums_kernel(const double* __restrict__ part, const double* __restrict__ row_sums,
                                                       double* __restrict__ sums, long n, int pc, int parts) {
  __shared__ double red[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  double T = 0.0, sxx = 0.0, sxy = 0.0;
  for (long i = tid; i < n; i += 256) T += row_sums[i];
  for (int k = tid; k < parts; k += 256) {
    sxx += part[2 * ((size_t)k * pc + b)];
    sxy += part[2 * ((size_t)k * pc + b) + 1];
  }
  T = md_block_sum(T, red);
  sxx = md_block_sum(sxx, red);
  sxy = md_block_sum(sxy, red);
  if (tid == 0) {
    sums[3 * (size_t)b + 0] = sxx;
    sums[3 * (size_t)b + 1] = (T - sxx) - 2.0 * sxy;
    sums[3 * (size_t)b + 2] = sxy;
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" int mmvae_mmd_chunks(long n) {
  if (!md_shape_ok(n, 1, 0)) return 0;
  int tpc, nc;
  md_plan(n, 0, &tpc, &nc);
  return nc;
}

extern "C" size_t mmvae_mmd_ws_doubles(long n, int D, int P, int chunks) {
  if (!md_shape_ok(n, D, P) || chunks < 0) return 0;
  int tpc, nc;
  md_plan(n, chunks, &tpc, &nc);
  return md_ws(n, D, P, nc).total;
}

extern "C" int mmvae_mmd_sums(const float* X, const float* Y, const unsigned char* member, double* ws, double* sums,
                              double* row_sums, long n_x, long n_y, int D, int P, int family, const double* params, int S,
                              int chunks, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && Y && ws && sums && row_sums && (member || P == 0));
  if (n_x < 2 || n_y < 2 || n_x > MMVAE_MMD_MAX_ROWS || n_y > MMVAE_MMD_MAX_ROWS || !md_shape_ok(n_x + n_y, D, P) ||
      chunks < 0 || family < MMVAE_MMD_RBF || family > MMVAE_MMD_ENERGY)
    return MMVAE_ERR_UNSUPPORTED;
  MdParams prm = {};
  if (family == MMVAE_MMD_ENERGY) {
    S = 0;
  } else {
    MMVAE_CHECK_ARG(params);
    if (S < 1 || S > MMVAE_MMD_MAX_SCALES) return MMVAE_ERR_UNSUPPORTED;
    for (int k = 0; k < S; ++k) {
      MMVAE_CHECK_ARG(isfinite(params[k]) && params[k] > 0.0);
      prm.p[k] = params[k];
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const long n = n_x + n_y;
  int tpc, nc;
  md_plan(n, chunks, &tpc, &nc);
  const MdWs w = md_ws(n, D, P, nc);
  const int rt = pt_tiles(n), pc = md_columns(P);
  double *prm_d = ws + w.prm, *mean = ws + w.mean, *n2 = ws + w.n2, *Z = ws + w.z, *rowpart = ws + w.rowpart,
         *part = ws + w.part;
  unsigned char* packed = reinterpret_cast<unsigned char*>(ws + w.packed);
  hipLaunchKernelGGL(mmd_mean_kernel, dim3(D), dim3(256), 0, s, X, Y, mean, prm_d, prm, n_x, n, D);
  hipLaunchKernelGGL(mmd_centre_kernel, dim3((unsigned)(((size_t)n * D + 255) / 256)), dim3(256), 0, s, X, Y, mean, Z, n_x,
                     n, D);
  hipLaunchKernelGGL(mmd_pack_kernel, dim3((unsigned)(((size_t)rt * pc * 4 + 255) / 256)), dim3(256), 0, s, member,
                     reinterpret_cast<uint4*>(packed), n_x, n, P, pc);
  hipLaunchKernelGGL(mmd_norm_kernel, dim3(rt), dim3(256), 0, s, Z, n2, n, D);
  const dim3 grid(nc, rt, pc / MMD_PB);
  if (family == MMVAE_MMD_RBF)
    hipLaunchKernelGGL((mmd_tile_kernel<MMVAE_MMD_RBF>), grid, dim3(256), 0, s, Z, n2, prm_d, packed, part, rowpart, n, D, S,
                       pc, tpc);
  else if (family == MMVAE_MMD_IMQ)
    hipLaunchKernelGGL((mmd_tile_kernel<MMVAE_MMD_IMQ>), grid, dim3(256), 0, s, Z, n2, prm_d, packed, part, rowpart, n, D, S,
                       pc, tpc);
  else
    hipLaunchKernelGGL((mmd_tile_kernel<MMVAE_MMD_ENERGY>), grid, dim3(256), 0, s, Z, n2, prm_d, packed, part, rowpart, n, D,
                       S, pc, tpc);
  hipLaunchKernelGGL(mmd_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rowpart, row_sums, n, nc);
  hipLaunchKernelGGL(mmd_sums_kernel, dim3(1 + P), dim3(256), 0, s, part, row_sums, sums, n, pc, rt * nc);
  return mmvae_launch_status();
}
