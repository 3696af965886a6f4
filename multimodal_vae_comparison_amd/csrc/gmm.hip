// Latent density estimation (TorchMMVAE.fit_latent_density / sample_latent_density): EM for a mixture
// of C Gaussians on fp32 rows converted on load, R restarts side by side, full or diagonal covariances, everything in double
// with scikit-learn's GaussianMixture arithmetic; the scoring of rows under given parameters; draws from a mixture.
//   gm_estep_kernel     per (restart, 64 rows): log p_ik = log w_k - (D log 2 pi + |(x_i - mu_k)^T P_k|^2) / 2 + sum_d log
//                       P_k[d, d] by the direct triangular product (P_k, upper triangular, packed in LDS beside the fp32 row
//                       tile; a thread owns two rows and every eighth column), norm_i = logsumexp_k, resp = exp(log p - norm),
//                       labels = the first largest log p.  In the fit it also writes what the M-step sums over rows start
//                       from: per block sum_i norm_i, sum_i r_ik and sum_i r_ik x_i over the block's rows in order.  The start
//                       of a fit runs it with resp = the one-hot of the given labels and no density.
//   gm_cov_kernel       per (chunk of 1024 rows, component, restart): n_k and mu_k from the blocks' partials in block order
//                       (every chunk computes the same bits; chunk 0 writes them), then the chunk's part of
//                       sum_i r_ik (x_i - mu_k)(x_i - mu_k)^T (full: a thread owns two rows and every eighth column of the
//                       D x D sum) or of sum_i r_ik x_i^2 (diag), rows in order.
//   gm_finish_kernel    per (component, restart): the chunks merged in order, / n_k, + reg_covar; the Cholesky factor L, the
//                       precision factor P = L^-T (forward substitution per column), sum_d log P[d, d]; the weights; workgroup
//                       0 of a restart merges the blocks' norm sums into the lower bound and keeps the restart's record.
//   gm_sample_kernel    one thread per draw: the component from u and the running sum of the weights, z = mu + L eps.
// An iteration is these three launches for all restarts together.  A restart's record (previous bound, n_iter, converged,
// a stamp of the iteration it finished at) and its components' Cholesky failures (a stamp per component) live in device
// memory; workgroups of a finished restart return at once, and a stamp written by a sibling workgroup of the same launch
// reads as "not finished" whether it is seen or not.  No kernel loops over iterations, no workgroup waits on another, no
// atomics; every sum over rows has one order (64-row blocks in order; 1024-row chunks in order): a restart's bits do not
// depend on the other restarts nor on how the host groups the iterations.
#include <float.h>
#include <math.h>

#include "common.hpp"

#define GM_ROWS 64                               // rows of an E-step workgroup
#define GM_Q 8                                   // threads per row pair: thread q owns the columns q, q + 8, ...
#define GM_PER (MMVAE_GMM_MAX_D / GM_Q)          // columns per thread at the most
#define GM_LDX (MMVAE_GMM_MAX_D + 1)             // padded row of a tile
#define GM_TRI (MMVAE_GMM_MAX_D * (MMVAE_GMM_MAX_D + 1) / 2)
#define GM_CHUNK 1024                            // rows of a covariance chunk
#define GM_STATE 4                               // doubles of a restart's record: previous bound, n_iter, converged, stamp
#define GM_LOG_2PI 1.8378770664093453            // log(2 pi)

static bool gm_rows_ok(long n) { return n >= 1 && n <= MMVAE_MANIFOLD_MAX_ROWS; }
static bool gm_model_ok(int D, int C, int R, int diag) {
  return D >= 1 && D <= MMVAE_GMM_MAX_D && C >= 1 && C <= MMVAE_CLUSTER_MAX_K && R >= 1 && R <= MMVAE_CLUSTER_MAX_INIT &&
         (diag == MMVAE_GMM_FULL || diag == MMVAE_GMM_DIAG);
}
static __host__ __device__ int gm_blocks(long n) { return (int)((n + GM_ROWS - 1) / GM_ROWS); }
static __host__ __device__ int gm_chunks(long n) { return (int)((n + GM_CHUNK - 1) / GM_CHUNK); }

// the workspace of a fit, in doubles: record | stamps | n_k | norm sums | moment partials | covariance partials
struct GmWs {
  double *state, *bad, *nk, *normpart, *mpart, *cpart;
  size_t total;
};
static GmWs gm_ws(double* ws, long rows, int D, int C, int R, int diag) {
  GmWs w;
  size_t o = 0;
  const size_t nblk = gm_blocks(rows), nch = gm_chunks(rows), el = diag ? D : (size_t)D * D;
  w.state = ws + o, o += (size_t)R * GM_STATE;
  w.bad = ws + o, o += (size_t)R * MMVAE_CLUSTER_MAX_K;
  w.nk = ws + o, o += (size_t)R * C;
  w.normpart = ws + o, o += (size_t)R * nblk;
  w.mpart = ws + o, o += (size_t)R * nblk * C * (D + 1);
  w.cpart = ws + o, o += (size_t)R * C * nch * el;
  w.total = o;
  return w;
}

// has restart r finished before iteration t?  (one thread asks; a stamp is the finishing iteration + 1, so that the stamps
// written during iteration t's own launches, t + 1, never count)
__device__ __forceinline__ bool gm_finished(const double* state, const double* bad, int r, int C, int t) {
  const double s = state[GM_STATE * r + 3];
  if (s != 0.0 && s <= (double)t) return true;
  for (int c = 0; c < C; ++c) {
    const double b = bad[(size_t)r * MMVAE_CLUSTER_MAX_K + c];
    if (b != 0.0 && b <= (double)t) return true;
  }
  return false;
}

// m^2 rounded on its own, never fused into the subtraction that follows: the diagonal variance sum r x^2 / n_k - mu^2 cancels,
// and numpy rounds mu^2 first (fused, a variance of reg_covar's size moves by ulp(mu^2) / reg_covar relative)
__device__ __forceinline__ double gm_square_rounded(double m) {
#pragma clang fp contract(off)
  return m * m;
}

// ---- E-step, scoring, and the one-hot start ------------------------------------------------------------------------------
struct GmEArgs {
  const float* X;
  const int* init;           // start: labels (R, N)
  const double *w, *mu, *prec, *logdet;
  double *resp, *logdens;    // (R, N, C) | (R, N); either may be NULL when scoring
  int* labels;               // (R, N) or NULL
  const double *state, *bad;
  double *normpart, *mpart;
  long N;
  int D, C, diag, mode, t;   // mode 0: iteration t of a fit; 1: the start; 2: scoring
};

// grid (ceil(N / 64), R), 256 threads: thread 8 rp + q owns the rows rp and rp + 32 of the block.  CP: the padded row of
// the log p / resp tile (C <= CP - 1).
template <int CP>
__global__ __launch_bounds__(256) void gm_estep_kernel(const GmEArgs a) {
  __shared__ float xs[GM_ROWS][GM_LDX];
  __shared__ double ps[GM_TRI];      // P_k: row i holds the columns i .. D - 1 from i D - i (i - 1) / 2; diag: the vector
  __shared__ double mus[MMVAE_GMM_MAX_D];
  __shared__ double lps[GM_ROWS][CP];
  __shared__ double nrm[GM_ROWS];
  __shared__ int sh;
  const int r = blockIdx.y, tid = threadIdx.x, rp = tid >> 3, q = tid & 7;
  const int D = a.D, C = a.C;
  const long N = a.N, i0 = (long)blockIdx.x * GM_ROWS;
  if (a.mode == 0) {
    if (tid == 0) sh = gm_finished(a.state, a.bad, r, C, a.t);
    __syncthreads();
    if (sh) return;
  }
  const int nvalid = (int)min((long)GM_ROWS, N - i0);
  for (int e = tid; e < GM_ROWS * D; e += 256) {
    const int rr = e / D, d = e % D;
    xs[rr][d] = rr < nvalid ? a.X[(size_t)(i0 + rr) * D + d] : 0.0f;
  }
  if (a.mode == 1) {
    for (int e = tid; e < GM_ROWS * C; e += 256) {
      const int rr = e / C, k = e % C;
      lps[rr][k] = (rr < nvalid && a.init[(size_t)r * N + i0 + rr] == k) ? 1.0 : 0.0;
    }
    __syncthreads();
  } else {
    const int per = (D + GM_Q - 1) / GM_Q;
    for (int k = 0; k < C; ++k) {
      const size_t rc = (size_t)r * C + k;
      __syncthreads();      // (the first: xs is staged; later ones: everybody is done with the previous P)
      if (a.diag) {
        if (tid < D) {
          ps[tid] = a.prec[rc * D + tid];
          mus[tid] = a.mu[rc * D + tid];
        }
      } else {
        const double* P = a.prec + rc * D * D;
        for (int e = tid; e < D * D; e += 256) {
          const int i = e / D, j = e % D;
          if (j >= i) ps[i * D - i * (i - 1) / 2 + j - i] = P[e];
        }
        if (tid < D) mus[tid] = a.mu[rc * D + tid];
      }
      __syncthreads();
      double s0 = 0.0, s1 = 0.0;
      if (a.diag) {
        for (int d = q; d < D; d += GM_Q) {
          const double y0 = ((double)xs[rp][d] - mus[d]) * ps[d], y1 = ((double)xs[rp + 32][d] - mus[d]) * ps[d];
          s0 += y0 * y0;
          s1 += y1 * y1;
        }
      } else {
        double y0[GM_PER], y1[GM_PER];
#pragma unroll
        for (int m = 0; m < GM_PER; ++m) y0[m] = y1[m] = 0.0;
        for (int i = 0; i < D; ++i) {
          const double m_i = mus[i];
          const double d0 = (double)xs[rp][i] - m_i, d1 = (double)xs[rp + 32][i] - m_i;
          const double* prow = ps + (i * D - i * (i - 1) / 2 - i);      // prow[j] = P[i, j], j >= i
#pragma unroll
          for (int m = 0; m < GM_PER; ++m) {
            const int j = q + GM_Q * m;
            if (m < per && j >= i && j < D) {
              const double p = prow[j];
              y0[m] += d0 * p;
              y1[m] += d1 * p;
            }
          }
        }
#pragma unroll
        for (int m = 0; m < GM_PER; ++m) {
          s0 += y0[m] * y0[m];      // (columns past D hold 0)
          s1 += y1[m] * y1[m];
        }
      }
      // the eight threads of a row pair are eight neighbouring lanes
#pragma unroll
      for (int o = 1; o < GM_Q; o <<= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
      }
      if (q == 0) {
        const double base = log(a.w[rc]) + a.logdet[rc];
        lps[rp][k] = -0.5 * ((double)D * GM_LOG_2PI + s0) + base;
        lps[rp + 32][k] = -0.5 * ((double)D * GM_LOG_2PI + s1) + base;
      }
    }
    __syncthreads();
    // norm_i = logsumexp_k, the first largest log p, resp in place of log p
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = rp + 32 * h;
      double best = -INFINITY;
      int bk = MMVAE_CLUSTER_MAX_K;
      for (int k = q; k < C; k += GM_Q) {
        const double v = lps[row][k];
        if (v > best) {
          best = v;
          bk = k;
        }
      }
#pragma unroll
      for (int o = 1; o < GM_Q; o <<= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int ok = __shfl_xor(bk, o, 64);
        if (ob > best || (ob == best && ok < bk)) {
          best = ob;
          bk = ok;
        }
      }
      double s = 0.0;
      for (int k = q; k < C; k += GM_Q) s += exp(lps[row][k] - best);
#pragma unroll
      for (int o = 1; o < GM_Q; o <<= 1) s += __shfl_xor(s, o, 64);
      const double norm = log(s) + best;
      for (int k = q; k < C; k += GM_Q) lps[row][k] = exp(lps[row][k] - norm);
      if (q == 0) {
        nrm[row] = norm;
        if (row < nvalid) {
          if (a.logdens) a.logdens[(size_t)r * N + i0 + row] = norm;
          if (a.labels) a.labels[(size_t)r * N + i0 + row] = bk < C ? bk : 0;
        }
      }
    }
    __syncthreads();
  }
  if (a.resp) {
    double* out = a.resp + ((size_t)r * N + i0) * C;      // (the block's rows are one contiguous run)
    for (int e = tid; e < nvalid * C; e += 256) out[e] = lps[e / C][e % C];
  }
  if (a.mode == 2) return;
  // what the M-step starts from: the block's sums over its rows, in order
  double* mp = a.mpart + ((size_t)r * gridDim.x + blockIdx.x) * C * (D + 1);
  for (int o = tid; o < C * (D + 1); o += 256) {
    const int k = o / (D + 1), d = o % (D + 1);
    double s = 0.0;
    for (int row = 0; row < nvalid; ++row) s += lps[row][k] * (d == D ? 1.0 : (double)xs[row][d]);
    mp[o] = s;
  }
  if (a.mode == 0 && tid == 0) {
    double s = 0.0;
    for (int row = 0; row < nvalid; ++row) s += nrm[row];
    a.normpart[(size_t)r * gridDim.x + blockIdx.x] = s;
  }
}

// ---- M-step: n_k, the means and the chunks' covariance sums ---------------------------------------------------------------
// grid (chunks, C, R), 256 threads: thread 8 ap + q owns the rows ap and ap + 32 and the columns q, q + 8, ... of the D x D
// sum (diag: thread d of wave w adds x_d^2 over the w-th quarter of the chunk; the quarters are added in order).
__global__ __launch_bounds__(256) void gm_cov_kernel(const float* __restrict__ X, const double* __restrict__ resp,
                                                     const double* __restrict__ mpart, const double* __restrict__ state,
                                                     const double* __restrict__ bad, double* __restrict__ nk,
                                                     double* __restrict__ means, double* __restrict__ cpart, long N, int D,
                                                     int C, int diag, int t) {
  __shared__ double ds[GM_ROWS][GM_LDX];
  __shared__ double rr[GM_ROWS];
  __shared__ double mus[MMVAE_GMM_MAX_D + 1];
  __shared__ int sh;
  const int chunk = blockIdx.x, c = blockIdx.y, r = blockIdx.z, tid = threadIdx.x;
  const int nblk = gm_blocks(N), nch = gridDim.x;
  if (t > 0) {
    if (tid == 0) sh = gm_finished(state, bad, r, C, t);
    __syncthreads();
    if (sh) return;
  }
  if (tid <= D) {
    const double* mp = mpart + ((size_t)r * nblk * C + c) * (D + 1) + tid;
    double s = 0.0;
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) s += mp[(size_t)b * C * (D + 1)];
    mus[tid] = s;
  }
  __syncthreads();
  const double n_k = mus[D] + 10.0 * DBL_EPSILON;
  __syncthreads();
  if (tid < D) {
    const double m = mus[tid] / n_k;
    mus[tid] = m;
    if (chunk == 0) means[((size_t)r * C + c) * D + tid] = m;
  }
  if (chunk == 0 && tid == 0) nk[(size_t)r * C + c] = n_k;
  __syncthreads();
  const long c0 = (long)chunk * GM_CHUNK, c1 = min(N, c0 + GM_CHUNK);
  const double* rs = resp + (size_t)r * N * C + c;
  if (diag) {
    const int wv = tid >> 6, d = tid & 63;
    const long q0 = c0 + (long)wv * (GM_CHUNK / 4), q1 = min(c1, q0 + GM_CHUNK / 4);
    double s = 0.0;
    if (d < D) {
#pragma unroll 4
      for (long i = q0; i < q1; ++i) {
        const double x = (double)X[(size_t)i * D + d];
        s += rs[(size_t)i * C] * (x * x);
      }
    }
    ds[wv][d] = s;
    __syncthreads();
    if (tid < D) cpart[(((size_t)r * C + c) * nch + chunk) * D + tid] = ((ds[0][tid] + ds[1][tid]) + ds[2][tid]) + ds[3][tid];
    return;
  }
  const int ap = tid >> 3, q = tid & 7, per = (D + GM_Q - 1) / GM_Q;
  double a0[GM_PER], a1[GM_PER];
#pragma unroll
  for (int m = 0; m < GM_PER; ++m) a0[m] = a1[m] = 0.0;
  for (long i0 = c0; i0 < c1; i0 += GM_ROWS) {
    const int nvalid = (int)min((long)GM_ROWS, c1 - i0);
    __syncthreads();
    for (int e = tid; e < GM_ROWS * D; e += 256) {
      const int row = e / D, d = e % D;
      ds[row][d] = row < nvalid ? (double)X[(size_t)(i0 + row) * D + d] - mus[d] : 0.0;
    }
    if (tid < GM_ROWS) rr[tid] = tid < nvalid ? rs[(size_t)(i0 + tid) * C] : 0.0;
    __syncthreads();
    if (ap < D) {
      const bool two = ap + 32 < D;
      for (int row = 0; row < nvalid; ++row) {
        const double w = rr[row];
        const double t0 = w * ds[row][ap], t1 = two ? w * ds[row][ap + 32] : 0.0;
#pragma unroll
        for (int m = 0; m < GM_PER; ++m)
          if (m < per) {
            const double b = ds[row][q + GM_Q * m];      // (columns past D: inside the padded row, never written out)
            a0[m] += t0 * b;
            a1[m] += t1 * b;
          }
      }
    }
  }
  double* out = cpart + (((size_t)r * C + c) * nch + chunk) * D * D;
#pragma unroll
  for (int m = 0; m < GM_PER; ++m) {
    const int b = q + GM_Q * m;
    if (b < D) {
      if (ap < D) out[ap * D + b] = a0[m];
      if (ap + 32 < D) out[(ap + 32) * D + b] = a1[m];
    }
  }
}

// ---- M-step: covariances, Cholesky and precision factors, weights, the restart's record ------------------------------------
// grid (C, R), 256 threads
__global__ __launch_bounds__(256) void gm_finish_kernel(const double* __restrict__ cpart, const double* __restrict__ nk,
                                                        const double* __restrict__ means,
                                                        const double* __restrict__ normpart, double* __restrict__ state,
                                                        double* __restrict__ bad, double* __restrict__ weights,
                                                        double* __restrict__ cov, double* __restrict__ chol,
                                                        double* __restrict__ prec, double* __restrict__ logdet, long N, int D,
                                                        int C, int diag, double reg, double tol, int t) {
  __shared__ double A[MMVAE_GMM_MAX_D][GM_LDX];      // the covariance's lower triangle, then L
  __shared__ double Z[MMVAE_GMM_MAX_D][GM_LDX];      // L^-1
  __shared__ double lg[MMVAE_GMM_MAX_D];
  __shared__ int sh, failed;
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const int nch = gm_chunks(N), nblk = gm_blocks(N);
  if (tid == 0) {
    sh = t > 0 && gm_finished(state, bad, r, C, t);
    failed = 0;
  }
  __syncthreads();
  if (sh) return;
  const size_t rc = (size_t)r * C + c;
  const double n_k = nk[rc];
  if (diag) {
    double v = 1.0;
    if (tid < D) {
      const double* part = cpart + rc * nch * D + tid;
      double s = 0.0;
      for (int h = 0; h < nch; ++h) s += part[(size_t)h * D];
      const double m = means[rc * D + tid];
      v = s / n_k - gm_square_rounded(m) + reg;
      cov[rc * D + tid] = v;
      const double sd = sqrt(v);
      chol[rc * D + tid] = sd;
      prec[rc * D + tid] = 1.0 / sd;
      lg[tid] = log(1.0 / sd);
    }
    if (!(v > 0.0) || !isfinite(v)) failed = 1;
  } else {
    const double* part = cpart + rc * nch * D * D;
    for (int e = tid; e < D * D; e += 256) {
      const int i = e / D, j = e % D;
      if (j <= i) {
        double s = 0.0;
        for (int h = 0; h < nch; ++h) s += part[(size_t)h * D * D + e];
        A[i][j] = s / n_k + (i == j ? reg : 0.0);
      }
    }
    __syncthreads();
    for (int e = tid; e < D * D; e += 256) {
      const int i = e / D, j = e % D;
      cov[rc * D * D + e] = j <= i ? A[i][j] : A[j][i];
    }
    // L, column by column: thread i owns row i
    for (int j = 0; j < D; ++j) {
      double s = 0.0;
      if (tid >= j && tid < D) {
        s = A[tid][j];
        for (int k = 0; k < j; ++k) s -= A[tid][k] * A[j][k];
        if (tid == j) {
          if (!(s > 0.0) || !isfinite(s)) failed = 1;
          A[j][j] = sqrt(s);
        }
      }
      __syncthreads();
      if (tid > j && tid < D) A[tid][j] = s / A[j][j];
      __syncthreads();
    }
    // L^-1 by forward substitution: thread j owns column j
    if (tid < D) {
      const int j = tid;
      Z[j][j] = 1.0 / A[j][j];
      for (int i = j + 1; i < D; ++i) {
        double s = 0.0;
        for (int k = j; k < i; ++k) s += A[i][k] * Z[k][j];
        Z[i][j] = (0.0 - s) / A[i][i];
      }
      lg[j] = log(Z[j][j]);
    }
    __syncthreads();
    for (int e = tid; e < D * D; e += 256) {
      const int i = e / D, j = e % D;
      chol[rc * D * D + e] = j <= i ? A[i][j] : 0.0;
      prec[rc * D * D + e] = j >= i ? Z[j][i] : 0.0;      // P = L^-T
    }
  }
  __syncthreads();
  if (tid != 0) return;
  double s = 0.0;
  for (int d = 0; d < D; ++d) s += lg[d];
  logdet[rc] = s;
  if (failed) bad[(size_t)r * MMVAE_CLUSTER_MAX_K + c] = (double)(t + 1);
  double total = 0.0;
  for (int k = 0; k < C; ++k) total += nk[(size_t)r * C + k] / (double)N;
  weights[rc] = (n_k / (double)N) / total;
  if (c == 0 && t > 0) {
    double lb = 0.0;
    for (int b = 0; b < nblk; ++b) lb += normpart[(size_t)r * nblk + b];
    lb /= (double)N;
    const double prev = t == 1 ? -INFINITY : state[GM_STATE * r];
    const bool conv = fabs(lb - prev) < tol;
    state[GM_STATE * r] = lb;
    state[GM_STATE * r + 1] = (double)t;
    state[GM_STATE * r + 2] = conv ? 1.0 : 0.0;
    if (conv) state[GM_STATE * r + 3] = (double)(t + 1);
  }
}

// ---- draws ---------------------------------------------------------------------------------------------------------------------
// one thread per draw; a single restart's parameters
__global__ __launch_bounds__(256) void gm_sample_kernel(const double* __restrict__ w, const double* __restrict__ mu,
                                                        const double* __restrict__ chol, const double* __restrict__ u,
                                                        const float* __restrict__ eps, float* __restrict__ z,
                                                        int* __restrict__ comp, long n, int D, int C, int diag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double ui = u[i];
  double cum = 0.0;
  int k = C - 1;
  for (int c = 0; c < C - 1; ++c) {
    cum += w[c];
    if (ui < cum) {
      k = c;
      break;
    }
  }
  comp[i] = k;
  const float* e = eps + (size_t)i * D;
  for (int d = 0; d < D; ++d) {
    double s;
    if (diag) {
      s = chol[(size_t)k * D + d] * (double)e[d];
    } else {
      const double* L = chol + ((size_t)k * D + d) * D;
      s = 0.0;
      for (int j = 0; j <= d; ++j) s += L[j] * (double)e[j];
    }
    z[(size_t)i * D + d] = (float)(mu[(size_t)k * D + d] + s);
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" size_t mmvae_gmm_ws_doubles(long rows, int D, int C, int restarts, int diag) {
  if (!gm_rows_ok(rows) || !gm_model_ok(D, C, restarts, diag)) return 0;
  return gm_ws(nullptr, rows, D, C, restarts, diag).total;
}

static void gm_launch_estep(const GmEArgs& a, int R, hipStream_t s) {
  const dim3 grid(gm_blocks(a.N), R);
  if (a.C <= 16)
    hipLaunchKernelGGL((gm_estep_kernel<17>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((gm_estep_kernel<MMVAE_CLUSTER_MAX_K + 1>), grid, dim3(256), 0, s, a);
}

extern "C" int mmvae_gmm_em(const float* X, const int* init, double* weights, double* means, double* cov, double* chol,
                            double* prec, double* logdet, double* resp, double* ws, long rows, int D, int C, int restarts,
                            int diag, double reg_covar, double tol, int it0, int n_iter, int max_iter,
                            mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && init && weights && means && cov && chol && prec && logdet && resp && ws);
  if (!gm_rows_ok(rows) || !gm_model_ok(D, C, restarts, diag) || max_iter < 1 || max_iter > MMVAE_CLUSTER_MAX_ITER ||
      it0 < 1 || n_iter < 1 || (long)it0 + n_iter - 1 > max_iter || !(reg_covar >= 0.0) || !(tol >= 0.0))
    return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const GmWs w = gm_ws(ws, rows, D, C, restarts, diag);
  GmEArgs a;
  a.X = X;
  a.init = init;
  a.w = weights;
  a.mu = means;
  a.prec = prec;
  a.logdet = logdet;
  a.resp = resp;
  a.logdens = nullptr;
  a.labels = nullptr;
  a.state = w.state;
  a.bad = w.bad;
  a.normpart = w.normpart;
  a.mpart = w.mpart;
  a.N = rows;
  a.D = D;
  a.C = C;
  a.diag = diag;
  const dim3 cgrid(gm_chunks(rows), C, restarts), fgrid(C, restarts);
  // the start (before iteration 1): the one-hot of the labels, then an M-step; numbered 0
  for (int t = it0 == 1 ? 0 : it0; t < it0 + n_iter; ++t) {
    a.mode = t == 0 ? 1 : 0;
    a.t = t;
    gm_launch_estep(a, restarts, s);
    hipLaunchKernelGGL(gm_cov_kernel, cgrid, dim3(256), 0, s, X, resp, w.mpart, w.state, w.bad, w.nk, means, w.cpart, rows, D,
                       C, diag, t);
    hipLaunchKernelGGL(gm_finish_kernel, fgrid, dim3(256), 0, s, w.cpart, w.nk, means, w.normpart, w.state, w.bad, weights,
                       cov, chol, prec, logdet, rows, D, C, diag, reg_covar, tol, t);
  }
  return mmvae_launch_status();
}

extern "C" int mmvae_gmm_score(const float* X, const double* weights, const double* means, const double* prec,
                               const double* logdet, double* logdens, double* resp, int* labels, long rows, int D, int C,
                               int restarts, int diag, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && weights && means && prec && logdet && logdens);
  if (!gm_rows_ok(rows) || !gm_model_ok(D, C, restarts, diag)) return MMVAE_ERR_UNSUPPORTED;
  GmEArgs a;
  a.X = X;
  a.init = nullptr;
  a.w = weights;
  a.mu = means;
  a.prec = prec;
  a.logdet = logdet;
  a.resp = resp;
  a.logdens = logdens;
  a.labels = labels;
  a.state = a.bad = nullptr;
  a.normpart = a.mpart = nullptr;
  a.N = rows;
  a.D = D;
  a.C = C;
  a.diag = diag;
  a.mode = 2;
  a.t = 0;
  gm_launch_estep(a, restarts, (hipStream_t)stream);
  return mmvae_launch_status();
}

extern "C" int mmvae_gmm_sample(const double* weights, const double* means, const double* chol, const double* u,
                                const float* eps, float* z, int* comp, long n, int D, int C, int diag, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(weights && means && chol && u && eps && z && comp);
  if (n < 1 || n > MMVAE_GMM_MAX_DRAWS || !gm_model_ok(D, C, 1, diag)) return MMVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gm_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, weights, means,
                     chol, u, eps, z, comp, n, D, C, diag);
  return mmvae_launch_status();
}
