// Latent cluster analysis (TorchMMVAE.cluster_latents): k-means (Lloyd) with many restarts side by side, the statistics of a
// partition and the silhouette sums, everything in double on fp32 rows converted on load.
//   cl_assign_kernel    per (restart, row) the squared distances to every centre by direct differences, features in order;
//                       the nearest centre (ties to the lowest index) or the distance to the row's own centre.  64 rows and a
//                       slab of 32 features of all centres are staged through LDS per step: any F with any C.
//   cl_means_kernel     per (restart, cluster) the count and the feature sums of its rows, one thread per feature, the rows
//                       walked in index order (a ballot over 64 labels at a time names them); a cluster without rows keeps
//                       what its centre held.
//   cl_spread_kernel    per (restart, cluster) the sums over its rows, in index order, of d^2 and of d; their sum over the
//                       clusters in order is the inertia.
//   The Lloyd driver is these launches: per iteration one assignment (labels in place; every workgroup records whether a
//   label of its rows changed) and one update (every workgroup reads the records of its restart: none set -> the restart
//   has converged, its first workgroup writes the state and no centre moves).  Workgroups of finished restarts return at
//   once.  No kernel loops over iterations and no workgroup waits on another; the host looks at the states every few
//   iterations (ops.kmeans_fit).
//   cl_sil_tile_kernel  the fp64 pair-tile walker of pair_tile.hpp with the rows addressed directly and the COLUMNS through
//                       a list of row numbers sorted by cluster, every cluster's run padded to whole 64-wide tiles with -1
//                       (zeros are staged, the epilogue skips them): a column tile belongs to one cluster.  The epilogue
//                       adds sqrt(max(0, |x_i|^2 + |x_j|^2 - 2 x_i . x_j)) over a tile's valid columns, the row's own
//                       number left out.  Workgroup (chunk, row tile) walks the tiles of one chunk of one cluster and writes
//                       one partial per row; neither the N x N matrix nor an N x n_c block is written.
//   cl_sil_merge_kernel the chunks of a cluster added in order into S (N, C)
// No atomics.  Every sum has one order that does not depend on the grid (k-means, statistics) or is fixed by the chunk plan
// (silhouette): two runs give the same bits.
#include <math.h>

#include "pair_tile.hpp"

#define CL_ROWS 64                              // rows of a workgroup of the assignment
#define CL_FS 32                                // features of a staged slab
#define CL_Q 4                                  // threads per row: thread q owns the centres q, q + 4, ...
#define CL_PER (MMVAE_CLUSTER_MAX_K / CL_Q)     // centres per thread at the most
#define CL_STATE 4                              // ints of a restart's state: finished, n_iter, converged, (unused)

static bool cl_rows_ok(long n) { return n >= 1 && n <= MMVAE_MANIFOLD_MAX_ROWS; }
static bool cl_f_ok(int F) { return F >= 1 && F <= MMVAE_FRECHET_MAX_F; }
static bool cl_k_ok(int C) { return C >= 1 && C <= MMVAE_CLUSTER_MAX_K; }
static bool cl_r_ok(int R) { return R >= 1 && R <= MMVAE_CLUSTER_MAX_INIT; }
static bool cl_shape_ok(long n, int F, int C, int R) { return cl_rows_ok(n) && cl_f_ok(F) && cl_k_ok(C) && cl_r_ok(R); }
static __host__ __device__ int cl_blocks(long n) { return (int)((n + CL_ROWS - 1) / CL_ROWS); }

// ---- assignment ----------------------------------------------------------------------------------------------------------
// grid (ceil(N / 64), R), 256 threads: thread 4 row + q.  mode 0: iteration t of the Lloyd loop (finished restarts return;
// labels in place; chg[r, block] = a label of the block's rows changed, or t == 1); mode 1: the nearest centre, labels and
// d2 written; mode 2: the labels are given, d2 = the squared distance to the row's own centre.
__global__ __launch_bounds__(256) void cl_assign_kernel(const float* __restrict__ X, const double* __restrict__ centres,
                                                        int* __restrict__ labels, double* __restrict__ d2out,
                                                        const int* __restrict__ state, int* __restrict__ chg, long N, int F,
                                                        int C, int mode, int t) {
  __shared__ float xs[CL_ROWS][CL_FS + 1];
  __shared__ double cs[MMVAE_CLUSTER_MAX_K][CL_FS + 1];
  const int r = blockIdx.y, tid = threadIdx.x, row = tid >> 2, q = tid & 3;
  if (mode == 0 && state[CL_STATE * r] != 0) return;      // (no launch of this kernel writes the state: uniform)
  const long i0 = (long)blockIdx.x * CL_ROWS;
  const double* mu = centres + (size_t)r * C * F;
  const int per = (C + CL_Q - 1) / CL_Q;
  const int srow = tid / CL_FS, sk = tid % CL_FS;
  double acc[CL_PER];
#pragma unroll
  for (int j = 0; j < CL_PER; ++j) acc[j] = 0.0;
  for (int k0 = 0; k0 < F; k0 += CL_FS) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < CL_ROWS * CL_FS / 256; ++e) {
      const int rr = srow + (256 / CL_FS) * e;
      xs[rr][sk] = (i0 + rr < N && k0 + sk < F) ? X[(size_t)(i0 + rr) * F + k0 + sk] : 0.0f;
      cs[rr][sk] = (rr < C && k0 + sk < F) ? mu[(size_t)rr * F + k0 + sk] : 0.0;
    }
    __syncthreads();
    // (features past F are zeros on both sides: they add +0.0)
    for (int k = 0; k < CL_FS; ++k) {
      const double xv = (double)xs[row][k];
#pragma unroll
      for (int j = 0; j < CL_PER; ++j)
        if (j < per) {
          const double d = xv - cs[q + CL_Q * j][k];
          acc[j] += d * d;
        }
    }
  }
  const long i = i0 + row;
  const int own = (mode == 2 && i < N) ? labels[(size_t)r * N + i] : -1;
  double best = INFINITY;
  int bc = MMVAE_CLUSTER_MAX_K;
#pragma unroll
  for (int j = 0; j < CL_PER; ++j) {
    const int c = q + CL_Q * j;
    if (mode == 2 ? c == own : (c < C && acc[j] < best)) {
      best = acc[j];
      bc = c;
    }
  }
  // the four threads of a row are four neighbouring lanes
#pragma unroll
  for (int o = 1; o < CL_Q; o <<= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(bc, o, 64);
    if (ob < best || (ob == best && oc < bc)) {
      best = ob;
      bc = oc;
    }
  }
  int changed = 0;
  if (q == 0 && i < N) {
    if (mode != 2) {
      changed = labels[(size_t)r * N + i] != bc;
      labels[(size_t)r * N + i] = bc;
    }
    if (d2out) d2out[(size_t)r * N + i] = best;
  }
  if (mode == 0) {
    const int any = __syncthreads_or(changed || t == 1);
    if (tid == 0) chg[(size_t)r * gridDim.x + blockIdx.x] = any;
  }
}

// ---- counts and means ------------------------------------------------------------------------------------------------------
// grid (C, R), 256 threads: thread tid owns the features tid + 256 e, e < E, of cluster c of restart r.  Every wave walks the
// rows in index order, 64 at a time: lane l reads the label of row i0 + l (the next 64 labels are on their way while these
// are used), a ballot gives the rows of the cluster, and their features are added in row order, G rows' loads in flight.
// t > 0, iteration t of the Lloyd loop: a finished restart returns; a restart none of whose blocks recorded a change has
// converged (workgroup 0 of the restart writes its state; a sibling that reads the state before or after that write does
// the same thing: nothing); a cluster without rows adds one to its own counter empties[r, c].
template <int E>
__global__ __launch_bounds__(256) void cl_means_kernel(const float* __restrict__ X, const int* __restrict__ labels,
                                                       double* __restrict__ centres, int* __restrict__ counts,
                                                       int* __restrict__ state, const int* __restrict__ chg,
                                                       int* __restrict__ empties, long N, int F, int C, int nblk, int t) {
  constexpr int G = E >= 4 ? 4 : 8;
  __shared__ int sh;
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  if (t > 0) {
    if (tid == 0) sh = state[CL_STATE * r];      // (one read for the workgroup: a sibling may be writing it)
    __syncthreads();
    if (sh != 0) return;
    int any = 0;
    for (int b = tid; b < nblk; b += 256) any |= chg[(size_t)r * nblk + b];
    if (!__syncthreads_or(any)) {
      if (c == 0 && tid == 0) {
        state[CL_STATE * r + 1] = t;
        state[CL_STATE * r + 2] = 1;
        state[CL_STATE * r] = 1;
      }
      return;
    }
  }
  if ((tid & ~63) >= F) return;      // (a wave without features; no barrier follows)
  const int* lab = labels + (size_t)r * N;
  double acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.0;
  int n = 0;
  int next = lane < N ? lab[lane] : -1;
  for (long i0 = 0; i0 < N; i0 += 64) {
    const int mine = next;
    next = i0 + 64 + lane < N ? lab[i0 + 64 + lane] : -1;
    unsigned long long rows = __ballot(mine == c);      // (the same for every lane: the loop below is uniform)
    n += __popcll(rows);
    while (rows) {
      int u[G];
      float v[G][E];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        u[g] = rows ? __ffsll(rows) - 1 : -1;
        rows &= rows - 1;
      }
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < E; ++e)
          v[g][e] = (u[g] >= 0 && tid + 256 * e < F) ? X[(size_t)(i0 + u[g]) * F + tid + 256 * e] : 0.0f;
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (u[g] >= 0) {
#pragma unroll
          for (int e = 0; e < E; ++e) acc[e] += (double)v[g][e];
        }
    }
  }
  if (n > 0) {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (tid + 256 * e < F) centres[((size_t)r * C + c) * F + tid + 256 * e] = acc[e] / (double)n;
  }
  if (tid == 0) {
    if (counts) counts[(size_t)r * C + c] = n;
    if (t > 0 && n == 0) empties[(size_t)r * MMVAE_CLUSTER_MAX_K + c] += 1;
  }
}

// ---- the spread of a partition -----------------------------------------------------------------------------------------------
// grid R, 64 threads: thread c adds d2[i] and sqrt(d2[i]) over the rows of cluster c in index order; thread 0 adds the
// clusters' sums of d2 in order: the inertia
__global__ __launch_bounds__(64) void cl_spread_kernel(const int* __restrict__ labels, const double* __restrict__ d2,
                                                       int* __restrict__ counts, double* __restrict__ within,
                                                       double* __restrict__ wdist, double* __restrict__ inertia, long N,
                                                       int C) {
  __shared__ double sw[MMVAE_CLUSTER_MAX_K];
  const int r = blockIdx.x, c = threadIdx.x;
  const int* lab = labels + (size_t)r * N;
  const double* d = d2 + (size_t)r * N;
  double w = 0.0, s = 0.0;
  int n = 0;
  for (long i = 0; i < N; ++i)
    if (lab[i] == c) {
      const double v = d[i];
      w += v;
      s += sqrt(v);
      ++n;
    }
  sw[c] = w;
  if (c < C) {
    counts[(size_t)r * C + c] = n;
    within[(size_t)r * C + c] = w;
    wdist[(size_t)r * C + c] = s;
  }
  __syncthreads();
  if (c == 0) {
    double total = 0.0;
    for (int k = 0; k < C; ++k) total += sw[k];
    inertia[r] = total;
  }
}

// ---- silhouette sums: the policies of pair_tile_walk -------------------------------------------------------------------------
// rows i0 + r of X addressed directly; the columns are the rows list[j0 + r] of X (-1, or a number outside the set: zeros
// are staged).  A thread keeps the eight row numbers it stages in registers, as kid.hip does.
struct ClRows {
  const float* X;
  const int* list;
  long i0, N, P;
  int F;
  int ra[PT_LOADS];      // (not initialised: columns() fills them before the first fetch)
  __device__ __forceinline__ ClRows(const float* X, const int* list, long i0, long N, long P, int F)
      : X(X), list(list), i0(i0), N(N), P(P), F(F) {}
  __device__ __forceinline__ void columns(long j0) {
    const int frow = threadIdx.x / PT_KT;
#pragma unroll
    for (int e = 0; e < PT_LOADS; ++e) {
      const long p = j0 + frow + (256 / PT_KT) * e;
      const int j = p < P ? list[p] : -1;
      ra[e] = (j >= 0 && j < N) ? j : -1;
    }
  }
  __device__ __forceinline__ float b(int e, int k0) const {
    const int r = threadIdx.x / PT_KT + (256 / PT_KT) * e, kk = threadIdx.x % PT_KT;
    return (k0 + kk < F && i0 + r < N) ? X[(size_t)(i0 + r) * F + k0 + kk] : 0.0f;
  }
  __device__ __forceinline__ float a(int e, long, int k0) const {
    const int kk = threadIdx.x % PT_KT;
    return (k0 + kk < F && ra[e] >= 0) ? X[(size_t)ra[e] * F + k0 + kk] : 0.0f;
  }
};

// d^2 from the norms and the dot product; a row's sum of the distances to the tile's valid columns, its own number left out
struct ClEpilogue {
  const double* n2;
  const int* list;
  long i0, N, P;
  double rowsum;
  __device__ __forceinline__ static int* col_s() {
    __shared__ int s[PT_TILE];
    return s;
  }
  __device__ __forceinline__ int col_of(long p) const {
    const int j = p < P ? list[p] : -1;
    return (j >= 0 && j < N) ? j : -1;
  }
  __device__ __forceinline__ void stage(int t) {
    if (threadIdx.x < PT_TILE) col_s()[threadIdx.x] = col_of((long)t * PT_TILE + threadIdx.x);
  }
  __device__ __forceinline__ double column(int t, int cj) const {
    const int j = col_of((long)t * PT_TILE + cj);
    return j >= 0 ? n2[j] : 0.0;
  }
  __device__ __forceinline__ double element(double ncol, int ci, double g) const {
    const double nrow = i0 + ci < N ? n2[i0 + ci] : 0.0;
    return fmax(0.0, (nrow + ncol) - 2.0 * g);
  }
  __device__ __forceinline__ void tile(const double* lds, int) {
    const int erow = threadIdx.x >> 2, equarter = threadIdx.x & 3;
    const long ei = i0 + erow;
    if (ei >= N) return;
#pragma unroll 4
    for (int c = equarter; c < PT_TILE; c += 4) {
      const int j = col_s()[c];
      if (j >= 0 && j != ei) rowsum += sqrt(lds[erow * PT_LDD + c]);
    }
  }
};

// grid (chunks, row tiles), 256 threads.  table (chunks, 3) = (cluster, first tile, tile past the last) of the padded list;
// part (chunks, N): the row's sum over the chunk's columns.
__global__ __launch_bounds__(256, 2) void cl_sil_tile_kernel(const float* __restrict__ X, const double* __restrict__ n2,
                                                            const int* __restrict__ list, const int* __restrict__ table,
                                                            double* __restrict__ part, long N, long P, int F) {
  const long i0 = (long)blockIdx.y * PT_TILE;
  const int tiles = pt_tiles(P);
  const int t0 = max(0, table[3 * blockIdx.x + 1]), t1 = min(tiles, table[3 * blockIdx.x + 2]);
  ClEpilogue epi{n2, list, i0, N, P, 0.0};
  pair_tile_walk(ClRows(X, list, i0, N, P, F), epi, F, t0, t1);
  // the four quarters of a row are four neighbouring lanes
#pragma unroll
  for (int o = 1; o < 4; o <<= 1) epi.rowsum += __shfl_xor(epi.rowsum, o, 64);
  const long ei = i0 + (threadIdx.x >> 2);
  if ((threadIdx.x & 3) == 0 && ei < N) part[(size_t)blockIdx.x * N + ei] = epi.rowsum;
}

// grid (ceil(N / 256), C): S[i, c] = the partials of the chunks [first[c], first[c + 1]) of cluster c, in order
__global__ __launch_bounds__(256) void cl_sil_merge_kernel(const double* __restrict__ part, const int* __restrict__ first,
                                                           double* __restrict__ S, long N, int C, int chunks) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= N) return;
  const int k0 = max(0, first[c]), k1 = min(chunks, first[c + 1]);
  double s = 0.0;
  for (int k = k0; k < k1; ++k) s += part[(size_t)k * N + i];
  S[(size_t)i * C + c] = s;
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" size_t mmvae_cluster_lloyd_ws_ints(long rows, int restarts) {
  if (!cl_rows_ok(rows) || !cl_r_ok(restarts)) return 0;
  return (size_t)restarts * (size_t)(CL_STATE + cl_blocks(rows) + MMVAE_CLUSTER_MAX_K);
}

extern "C" int mmvae_cluster_sil_tiles_per_chunk(long rows, int col_tiles, int chunks) {
  if (!cl_rows_ok(rows) || col_tiles < 1 || col_tiles > pt_tiles(MMVAE_MANIFOLD_MAX_ROWS) + MMVAE_CLUSTER_MAX_K || chunks < 0)
    return 0;
  int tpc, n;
  pair_plan(pt_tiles(rows), col_tiles, chunks, PT_SLOTS, PT_MIN_TILES, &tpc, &n);
  return tpc;
}

extern "C" size_t mmvae_cluster_sil_ws_doubles(long rows, int chunks) {
  if (!cl_rows_ok(rows) || chunks < 1 || chunks > pt_tiles(MMVAE_MANIFOLD_MAX_ROWS) + MMVAE_CLUSTER_MAX_K) return 0;
  return (size_t)chunks * (size_t)rows;
}

static void cl_launch_means(const float* X, const int* labels, double* centres, int* counts, int* state, const int* chg,
                            int* empties, long rows, int F, int C, int R, int t, hipStream_t s) {
  const dim3 grid(C, R);
  const int nblk = cl_blocks(rows);
  if (F <= 256)
    hipLaunchKernelGGL((cl_means_kernel<1>), grid, dim3(256), 0, s, X, labels, centres, counts, state, chg, empties, rows, F,
                       C, nblk, t);
  else if (F <= 512)
    hipLaunchKernelGGL((cl_means_kernel<2>), grid, dim3(256), 0, s, X, labels, centres, counts, state, chg, empties, rows, F,
                       C, nblk, t);
  else if (F <= 1024)
    hipLaunchKernelGGL((cl_means_kernel<4>), grid, dim3(256), 0, s, X, labels, centres, counts, state, chg, empties, rows, F,
                       C, nblk, t);
  else
    hipLaunchKernelGGL((cl_means_kernel<8>), grid, dim3(256), 0, s, X, labels, centres, counts, state, chg, empties, rows, F,
                       C, nblk, t);
}

extern "C" int mmvae_cluster_assign(const float* X, const double* centres, int* labels, double* d2, long rows, int F, int C,
                                    int restarts, int given, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && centres && labels && d2);
  if (!cl_shape_ok(rows, F, C, restarts) || given < 0 || given > 1) return MMVAE_ERR_UNSUPPORTED;
  const int* no_state = nullptr;
  int* no_chg = nullptr;
  hipLaunchKernelGGL(cl_assign_kernel, dim3(cl_blocks(rows), restarts), dim3(256), 0, (hipStream_t)stream, X, centres, labels,
                     d2, no_state, no_chg, rows, F, C, given ? 2 : 1, 0);
  return mmvae_launch_status();
}

extern "C" int mmvae_cluster_means(const float* X, const int* labels, double* means, int* counts, long rows, int F, int C,
                                   int restarts, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && labels && means && counts);
  if (!cl_shape_ok(rows, F, C, restarts)) return MMVAE_ERR_UNSUPPORTED;
  cl_launch_means(X, labels, means, counts, nullptr, nullptr, nullptr, rows, F, C, restarts, 0, (hipStream_t)stream);
  return mmvae_launch_status();
}

extern "C" int mmvae_cluster_spread(const int* labels, const double* d2, int* counts, double* within, double* wdist,
                                    double* inertia, long rows, int C, int restarts, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(labels && d2 && counts && within && wdist && inertia);
  if (!cl_rows_ok(rows) || !cl_k_ok(C) || !cl_r_ok(restarts)) return MMVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(cl_spread_kernel, dim3(restarts), dim3(MMVAE_CLUSTER_MAX_K), 0, (hipStream_t)stream, labels, d2, counts,
                     within, wdist, inertia, rows, C);
  return mmvae_launch_status();
}

extern "C" int mmvae_cluster_lloyd(const float* X, double* centres, int* labels, int* ws, long rows, int F, int C,
                                   int restarts, int it0, int n_iter, int max_iter, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && centres && labels && ws);
  if (!cl_shape_ok(rows, F, C, restarts) || max_iter < 1 || max_iter > MMVAE_CLUSTER_MAX_ITER || it0 < 1 || n_iter < 1 ||
      (long)it0 + n_iter - 1 > max_iter)
    return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int* state = ws;
  int* chg = ws + (size_t)CL_STATE * restarts;
  int* empties = chg + (size_t)restarts * cl_blocks(rows);
  double* no_d2 = nullptr;
  int* no_counts = nullptr;
  for (int t = it0; t < it0 + n_iter; ++t) {
    hipLaunchKernelGGL(cl_assign_kernel, dim3(cl_blocks(rows), restarts), dim3(256), 0, s, X, centres, labels, no_d2, state,
                       chg, rows, F, C, 0, t);
    cl_launch_means(X, labels, centres, no_counts, state, chg, empties, rows, F, C, restarts, t, s);
  }
  return mmvae_launch_status();
}

extern "C" int mmvae_cluster_sil_sums(const float* X, const double* n2, const int* list, const int* table, const int* first,
                                      double* ws, double* S, long rows, int F, int C, long padded, int chunks,
                                      mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && n2 && list && table && first && ws && S);
  if (!cl_rows_ok(rows) || !cl_f_ok(F) || !cl_k_ok(C) || padded < 1 || padded % PT_TILE != 0 ||
      padded > (long)PT_TILE * (pt_tiles(rows) + C) || chunks < 1 || chunks > pt_tiles(padded))
    return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cl_sil_tile_kernel, dim3(chunks, pt_tiles(rows)), dim3(256), 0, s, X, n2, list, table, ws, rows, padded, F);
  hipLaunchKernelGGL(cl_sil_merge_kernel, dim3((unsigned)((rows + 255) / 256), C), dim3(256), 0, s, ws, first, S, rows, C,
                     chunks);
  return mmvae_launch_status();
}
