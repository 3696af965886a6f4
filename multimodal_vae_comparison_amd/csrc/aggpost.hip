// Aggregate posterior of the latent code (TorchMMVAE.disentanglement; ops.aggregate_posterior): log q(z_n), log q(z_nd) and
// the class-conditional log q(z_nd | v_k = v_k(n)) of q(z) = (1/N) sum_m q(z | x_m) at every sample -- what the ELBO
// decomposition (index-code MI, total correlation, dimension-wise KL; Chen et al. 2018) and the mutual information gap read.
// Pair term in double from fp32 inputs converted on load, t = (z_nd - loc_md) / s_md:
//   Normal  l[n,m,d] = -t^2 / 2 - log s_md - log(2 pi) / 2        Laplace  l[n,m,d] = -|t| - log(2 s_md)
//   ap_shift_kernel     shift[n,d] = l[n,n,d] and jshift[n] = sum_d l[n,n,d] (d in order), one thread per row
//   ap_marginal_kernel  a workgroup owns 64 sample rows (one per lane), 16 dimensions (4 per wave) and a chunk of posterior
//                       rows, staged 32 at a time in LDS as (loc, 1/s, -log s - const) with their labels; a thread keeps
//                       4 x (1 + K) plain fp64 sums of exp(l - shift): ONE exp per (n, m, d), the K class sums reuse it
//                       through a select on labels[k,m] == labels[k,n]
//   ap_joint_kernel     the same rows and chunk, every dimension: wave q of a workgroup owns 8 of the 32 staged posterior
//                       rows, a thread adds l over d in order in a register per (n, m) (no sum over lanes, no exp per d) and
//                       takes one exp per (n, m); it also counts the class sizes (integers); the four waves' sums are added
//                       in wave order through LDS
//   ap_merge_kernel     the chunks' partials added in chunk order, then shift + log(sum) - log(count)
// The N x N x D terms are never written.  No atomics; every sum has one order for a given plan: two runs give the same
// bits, two plans regroup fp64 sums.  The fixed shift: row n is one of the m (of its own class too), so that the sums
// hold the term exp(0) = 1 and cannot vanish; the argument is bounded by the row's own standardised residual plus
// log(s_n / s_m) and cannot overflow for a z drawn from its posterior.
#include <math.h>

#include "common.hpp"

#define AP_ROWS 64                 // sample rows of a workgroup: one per lane
#define AP_DB 4                    // dimensions of a thread of the marginal kernel
#define AP_DW (4 * AP_DB)          // dimensions of a workgroup of the marginal kernel
#define AP_MT 32                   // posterior rows of a staged tile
#define AP_JD 32                   // dimensions of a staged step of the joint kernel
#define AP_JR (AP_MT / 4)          // posterior rows of a wave of the joint kernel
#define AP_SLOTS 2048              // workgroups wanted: 256 CUs x 8 (3 - 6 resident per CU: two rounds even the tail out)
#define AP_MIN_TILES 2             // staged tiles per chunk at least
#define AP_MAX_D 256
#define AP_KK MMVAE_AGGPOST_MAX_FACTORS
#define AP_HALF_LOG_2PI 0.91893853320467274178

static bool ap_ok(long N, int D, int K, int chunks) {
  return N >= 1 && N <= MMVAE_AGGPOST_MAX_ROWS && D >= 1 && D <= AP_MAX_D && K >= 0 && K <= AP_KK && chunks >= 0;
}
static int ap_row_tiles(long N) { return (int)((N + AP_ROWS - 1) / AP_ROWS); }
static int ap_dim_blocks(int D) { return (D + AP_DW - 1) / AP_DW; }

// -> staged tiles per chunk and the chunks that hold at least one tile; `chunks` 0: the default plan
static void ap_plan(long N, int D, int chunks, int* tiles_per_chunk, int* n_chunks) {
  const int pt = (int)((N + AP_MT - 1) / AP_MT);
  if (chunks <= 0) {
    const int wg = ap_row_tiles(N) * ap_dim_blocks(D);
    chunks = (AP_SLOTS + wg - 1) / wg;
    const int most = (pt + AP_MIN_TILES - 1) / AP_MIN_TILES;
    if (chunks > most) chunks = most;
  }
  if (chunks > pt) chunks = pt;
  *tiles_per_chunk = (pt + chunks - 1) / chunks;
  *n_chunks = (pt + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

// what a posterior row gives every pair: 1 / s and -log s - the family's constant
template <bool LAPLACE>
__device__ __forceinline__ void ap_row_terms(float scale, double* inv, double* c) {
  const double s = (double)scale;
  *inv = 1.0 / s;
  *c = LAPLACE ? -log(2.0 * s) : -log(s) - AP_HALF_LOG_2PI;
}
template <bool LAPLACE>
__device__ __forceinline__ double ap_term(double z, double loc, double inv, double c) {
  const double t = (z - loc) * inv;
  return LAPLACE ? c - fabs(t) : c - 0.5 * (t * t);
}

// ---- the shifts: one thread per row -------------------------------------------------------------------------------------
template <bool LAPLACE>
__global__ __launch_bounds__(256) void ap_shift_kernel(const float* __restrict__ z, const float* __restrict__ loc,
                                                       const float* __restrict__ scale, double* __restrict__ shift,
                                                       double* __restrict__ jshift, long N, int D) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double sum = 0.0;
  for (int d = 0; d < D; ++d) {
    const size_t at = (size_t)n * D + d;
    double inv, c;
    ap_row_terms<LAPLACE>(scale[at], &inv, &c);
    const double l = ap_term<LAPLACE>((double)z[at], (double)loc[at], inv, c);
    shift[at] = l;
    sum += l;
  }
  jshift[n] = sum;
}

// ---- log q(z_nd) and its class-conditional forms ---------------------------------------------------------------------------
// grid (chunks, row tiles, dimension blocks), 256 threads: lane = row, wave = 4 dimensions.  Every LDS read of the inner
// loop is a broadcast (all lanes of a wave read one posterior row's values).
// part (chunk, n, d, 1 + K): the chunk's sums of exp(l - shift), all rows first, then the rows of n's class per factor
template <bool LAPLACE, int KK>
__global__ __launch_bounds__(256) void ap_marginal_kernel(const float* __restrict__ z, const float* __restrict__ loc,
                                                          const float* __restrict__ scale, const int* __restrict__ labels,
                                                          const double* __restrict__ shift, double* __restrict__ part,
                                                          long N, int D, int K, int tpc) {
  __shared__ double loc_s[AP_MT][AP_DW], inv_s[AP_MT][AP_DW], c_s[AP_MT][AP_DW];
  __shared__ int lab_s[AP_MT][KK > 0 ? KK : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = (long)blockIdx.y * AP_ROWS + lane;
  const int dw0 = blockIdx.z * AP_DW, d0 = dw0 + wave * AP_DB;
  const bool live = n < N;
  double zz[AP_DB], sh[AP_DB], acc[AP_DB][1 + KK];
  int mine[KK > 0 ? KK : 1];
#pragma unroll
  for (int j = 0; j < AP_DB; ++j) {
    const bool in = live && d0 + j < D;
    zz[j] = in ? (double)z[(size_t)n * D + d0 + j] : 0.0;
    sh[j] = in ? shift[(size_t)n * D + d0 + j] : 0.0;
#pragma unroll
    for (int a = 0; a < 1 + KK; ++a) acc[j][a] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < KK; ++k) mine[k] = (live && k < K) ? labels[(size_t)k * N + n] : -1;
  const int pt = (int)((N + AP_MT - 1) / AP_MT);
  const int t0 = blockIdx.x * tpc, t1 = min(pt, t0 + tpc);
  for (int t = t0; t < t1; ++t) {
    const long m0 = (long)t * AP_MT;
    __syncthreads();        // (the previous tile has been read)
#pragma unroll
    for (int e = 0; e < AP_MT * AP_DW / 256; ++e) {
      const int idx = tid + 256 * e, r = idx / AP_DW, dd = idx % AP_DW;
      double lo = 0.0, inv = 0.0, c = 0.0;
      if (m0 + r < N && dw0 + dd < D) {
        const size_t at = (size_t)(m0 + r) * D + dw0 + dd;
        lo = (double)loc[at];
        ap_row_terms<LAPLACE>(scale[at], &inv, &c);
      }
      loc_s[r][dd] = lo;
      inv_s[r][dd] = inv;
      c_s[r][dd] = c;
    }
    if (KK > 0) {
      static_assert(AP_MT * (KK > 0 ? KK : 1) <= 256, "one label per thread");
      if (tid < AP_MT * KK) {
        const int r = tid / (KK > 0 ? KK : 1), k = tid % (KK > 0 ? KK : 1);
        lab_s[r][k] = (k < K && m0 + r < N) ? labels[(size_t)k * N + m0 + r] : -2;
      }
    }
    __syncthreads();
    const int rows = (int)min((long)AP_MT, N - m0);
    for (int r = 0; r < rows; ++r) {
      bool same[KK > 0 ? KK : 1];
#pragma unroll
      for (int k = 0; k < KK; ++k) same[k] = lab_s[r][k] == mine[k];
#pragma unroll
      for (int j = 0; j < AP_DB; ++j) {
        const int dd = wave * AP_DB + j;
        const double e = exp(ap_term<LAPLACE>(zz[j], loc_s[r][dd], inv_s[r][dd], c_s[r][dd]) - sh[j]);
        acc[j][0] += e;
#pragma unroll
        for (int k = 0; k < KK; ++k) acc[j][1 + k] += same[k] ? e : 0.0;
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < AP_DB; ++j) {
    if (d0 + j >= D) continue;
    double* out = part + (((size_t)blockIdx.x * N + n) * D + d0 + j) * (1 + K);
    out[0] = acc[j][0];
#pragma unroll
    for (int k = 0; k < KK; ++k)
      if (k < K) out[1 + k] = acc[j][1 + k];
  }
}

// ---- log q(z_n) and the class sizes ----------------------------------------------------------------------------------------
// grid (chunks, row tiles), 256 threads: lane = row, wave q = the staged posterior rows [8 q, 8 q + 8).  Per staged tile
// the dimensions go through LDS AP_JD at a time (the rows' own z beside them, fp32, odd row stride); lsum[i] holds
// sum_d l of (row, posterior row 8 q + i), d in order.
// part (chunk, n, 1 + K): the chunk's sum of exp(sum_d l - jshift), then the members of n's class per factor met in it
template <bool LAPLACE, int KK>
__global__ __launch_bounds__(256) void ap_joint_kernel(const float* __restrict__ z, const float* __restrict__ loc,
                                                       const float* __restrict__ scale, const int* __restrict__ labels,
                                                       const double* __restrict__ jshift, double* __restrict__ part, long N,
                                                       int D, int K, int tpc) {
  __shared__ double stage[3 * AP_MT * AP_JD];
  __shared__ float z_s[AP_ROWS][AP_JD + 1];
  __shared__ int lab_s[AP_MT][KK > 0 ? KK : 1];
  double(*loc_s)[AP_JD] = reinterpret_cast<double(*)[AP_JD]>(stage);
  double(*inv_s)[AP_JD] = reinterpret_cast<double(*)[AP_JD]>(stage + AP_MT * AP_JD);
  double(*c_s)[AP_JD] = reinterpret_cast<double(*)[AP_JD]>(stage + 2 * AP_MT * AP_JD);
  static_assert(4 * AP_ROWS * (1 + KK) <= 3 * AP_MT * AP_JD, "the waves' sums fit inside the staged tile");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n0 = (long)blockIdx.y * AP_ROWS, n = n0 + lane;
  const bool live = n < N;
  const double jsh = live ? jshift[n] : 0.0;
  int mine[KK > 0 ? KK : 1];
#pragma unroll
  for (int k = 0; k < KK; ++k) mine[k] = (live && k < K) ? labels[(size_t)k * N + n] : -1;
  double jacc = 0.0;
  int count[KK > 0 ? KK : 1];
#pragma unroll
  for (int k = 0; k < (KK > 0 ? KK : 1); ++k) count[k] = 0;
  const int pt = (int)((N + AP_MT - 1) / AP_MT);
  const int t0 = blockIdx.x * tpc, t1 = min(pt, t0 + tpc);
  for (int t = t0; t < t1; ++t) {
    const long m0 = (long)t * AP_MT;
    double lsum[AP_JR];
#pragma unroll
    for (int i = 0; i < AP_JR; ++i) lsum[i] = 0.0;
    for (int db = 0; db < D; db += AP_JD) {
      __syncthreads();      // (the previous step, and the previous tile's labels, have been read)
#pragma unroll
      for (int e = 0; e < AP_MT * AP_JD / 256; ++e) {
        const int idx = tid + 256 * e, r = idx / AP_JD, dd = idx % AP_JD;
        double lo = 0.0, inv = 0.0, c = 0.0;
        if (m0 + r < N && db + dd < D) {
          const size_t at = (size_t)(m0 + r) * D + db + dd;
          lo = (double)loc[at];
          ap_row_terms<LAPLACE>(scale[at], &inv, &c);
        }
        loc_s[r][dd] = lo;
        inv_s[r][dd] = inv;
        c_s[r][dd] = c;
      }
#pragma unroll
      for (int e = 0; e < AP_ROWS * AP_JD / 256; ++e) {
        const int idx = tid + 256 * e, r = idx / AP_JD, dd = idx % AP_JD;
        z_s[r][dd] = (n0 + r < N && db + dd < D) ? z[(size_t)(n0 + r) * D + db + dd] : 0.0f;
      }
      if (KK > 0 && db == 0 && tid < AP_MT * KK) {
        const int r = tid / (KK > 0 ? KK : 1), k = tid % (KK > 0 ? KK : 1);
        lab_s[r][k] = (k < K && m0 + r < N) ? labels[(size_t)k * N + m0 + r] : -2;
      }
      __syncthreads();
      const int dims = min(AP_JD, D - db);
      for (int dd = 0; dd < dims; ++dd) {
        const double zv = (double)z_s[lane][dd];
#pragma unroll
        for (int i = 0; i < AP_JR; ++i) {
          const int r = wave * AP_JR + i;
          lsum[i] += ap_term<LAPLACE>(zv, loc_s[r][dd], inv_s[r][dd], c_s[r][dd]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < AP_JR; ++i) {
      const int r = wave * AP_JR + i;
      if (m0 + r < N) {
        jacc += exp(lsum[i] - jsh);
#pragma unroll
        for (int k = 0; k < KK; ++k) count[k] += lab_s[r][k] == mine[k] ? 1 : 0;
      }
    }
  }
  __syncthreads();          // (the last step has been read: the waves' sums take the staged tile's place)
  double* red = stage + ((size_t)wave * AP_ROWS + lane) * (1 + KK);
  red[0] = jacc;
#pragma unroll
  for (int k = 0; k < KK; ++k) red[1 + k] = (double)count[k];
  __syncthreads();
  if (wave == 0 && live) {
    double* out = part + ((size_t)blockIdx.x * N + n) * (1 + K);
#pragma unroll
    for (int a = 0; a < 1 + KK; ++a) {
      if (a > K) continue;
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) s += stage[((size_t)q * AP_ROWS + lane) * (1 + KK) + a];
      out[a] = s;
    }
  }
}

// ---- the chunks in order, then shift + log(sum) - log(count): one thread per (n, d), d == D the joint ------------------------
__global__ __launch_bounds__(256) void ap_merge_kernel(const double* __restrict__ shift, const double* __restrict__ jshift,
                                                       const double* __restrict__ mpart, const double* __restrict__ jpart,
                                                       double* __restrict__ joint, double* __restrict__ marginal,
                                                       double* __restrict__ conditional, long N, int D, int K, int chunks) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * (D + 1)) return;
  const long n = idx / (D + 1);
  const int d = (int)(idx % (D + 1));
  const double log_n = log((double)N);
  if (d == D) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += jpart[((size_t)c * N + n) * (1 + K)];
    joint[n] = jshift[n] + log(s) - log_n;
    return;
  }
  const double sh = shift[(size_t)n * D + d];
  for (int a = 0; a < 1 + K; ++a) {
    double s = 0.0, members = 0.0;
    for (int c = 0; c < chunks; ++c) {
      s += mpart[(((size_t)c * N + n) * D + d) * (1 + K) + a];
      if (a > 0) members += jpart[((size_t)c * N + n) * (1 + K) + a];
    }
    if (a == 0)
      marginal[(size_t)n * D + d] = sh + log(s) - log_n;
    else
      conditional[((size_t)(a - 1) * N + n) * D + d] = sh + log(s) - log(members);
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" int mmvae_aggpost_chunks(long N, int D) {
  if (!ap_ok(N, D, 0, 0)) return 0;
  int tpc, n;
  ap_plan(N, D, 0, &tpc, &n);
  return n;
}

extern "C" size_t mmvae_aggpost_ws_doubles(long N, int D, int K, int chunks) {
  if (!ap_ok(N, D, K, chunks)) return 0;
  int tpc, n;
  ap_plan(N, D, chunks, &tpc, &n);
  return (size_t)N * D + (size_t)N + (size_t)n * N * (1 + K) * ((size_t)D + 1);
}

template <bool LAPLACE>
static void ap_launch(const float* z, const float* loc, const float* scale, const int* labels, double* ws, double* joint,
                      double* marginal, double* conditional, long N, int D, int K, int tpc, int n, hipStream_t s) {
  double* shift = ws;
  double* jshift = shift + (size_t)N * D;
  double* mpart = jshift + N;
  double* jpart = mpart + (size_t)n * N * D * (1 + K);
  hipLaunchKernelGGL((ap_shift_kernel<LAPLACE>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, z, loc, scale, shift,
                     jshift, N, D);
  const dim3 mgrid(n, ap_row_tiles(N), ap_dim_blocks(D)), jgrid(n, ap_row_tiles(N));
  if (K > 0) {
    hipLaunchKernelGGL((ap_marginal_kernel<LAPLACE, AP_KK>), mgrid, dim3(256), 0, s, z, loc, scale, labels, shift, mpart, N,
                       D, K, tpc);
    hipLaunchKernelGGL((ap_joint_kernel<LAPLACE, AP_KK>), jgrid, dim3(256), 0, s, z, loc, scale, labels, jshift, jpart, N, D,
                       K, tpc);
  } else {
    hipLaunchKernelGGL((ap_marginal_kernel<LAPLACE, 0>), mgrid, dim3(256), 0, s, z, loc, scale, labels, shift, mpart, N, D, K,
                       tpc);
    hipLaunchKernelGGL((ap_joint_kernel<LAPLACE, 0>), jgrid, dim3(256), 0, s, z, loc, scale, labels, jshift, jpart, N, D, K,
                       tpc);
  }
  hipLaunchKernelGGL(ap_merge_kernel, dim3((unsigned)((N * (D + 1) + 255) / 256)), dim3(256), 0, s, shift, jshift, mpart,
                     jpart, joint, marginal, conditional, N, D, K, n);
}

extern "C" int mmvae_aggpost_lse(const float* z, const float* loc, const float* scale, int laplace, const int* labels,
                                 double* ws, double* joint, double* marginal, double* conditional, long N, int D, int K,
                                 int chunks, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(z && loc && scale && ws && joint && marginal);
  if (!ap_ok(N, D, K, chunks)) return MMVAE_ERR_UNSUPPORTED;
  MMVAE_CHECK_ARG(K == 0 || (labels && conditional));
  int tpc, n;
  ap_plan(N, D, chunks, &tpc, &n);
  if (laplace)
    ap_launch<true>(z, loc, scale, labels, ws, joint, marginal, conditional, N, D, K, tpc, n, (hipStream_t)stream);
  else
    ap_launch<false>(z, loc, scale, labels, ws, joint, marginal, conditional, N, D, K, tpc, n, (hipStream_t)stream);
  return mmvae_launch_status();
}
