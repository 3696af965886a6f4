// Latent analysis (TorchMMVAE.analyse_latents): exact t-SNE of the latent samples, every pair term of every iteration
// on chip.  The arithmetic is scikit-learn's method="exact" path (manifold/_utils.pyx: _binary_search_perplexity;
// manifold/_t_sne.py: _joint_probabilities, _kl_divergence, _gradient_descent), restated in include/mmvae_hip.h.
//   once per embedding (cost irrelevant next to the iterations, everything in double):
//     tsne_sqdist_kernel   D2 = direct sums of squared differences, rounded to fp32
//     tsne_search_kernel   one workgroup per row: the binary search for the row's precision beta
//     tsne_psum_kernel     sum P = 2 sum_i (row sum of the conditional P), one workgroup, fixed order
//     tsne_joint_kernel    P_ij = max((c_ij + c_ji) / sum P, eps), both conditional terms recomputed from (beta, s)
//   per iteration, two launches:
//     tsne_forces_kernel   one WAVE per 4 rows streams every column: lanes own 4 consecutive columns (16-byte loads of
//                          the P tile, read exactly once; y_j loaded once per 4 rows), 4-term fp32 partials flushed into
//                          double accumulators, a fixed shuffle tree at the end of the rows -> 8 doubles per row
//     tsne_update_kernel   one workgroup: Z and the KL pieces reduced in a fixed order, g = 4 (ex attr - rep / Z), gains,
//                          momentum, y += upd, and the iteration's (KL, |g|) into the log
// No atomics, no cooperative launch: a row's sums are one wave's, the cross-row sums one workgroup's, so that two runs,
// and a run split over calls, give the same bits.
#include "common.hpp"

#define TSNE_EPS 2.220446049250313e-16
#define TSNE_RB 4             // rows per wave of the forces kernel
#define TSNE_FWAVES 4         // waves per workgroup of the forces kernel
#define TSNE_UPD_THREADS 1024
#define TSNE_ROW_DOUBLES 8    // per row: attr x, attr y, rep x, rep y, z, klA, klB, (unused)

__device__ __forceinline__ double tsne_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup (a multiple of 64 threads, at most 1024), the same value in every thread; red: 16 doubles
__device__ __forceinline__ double tsne_block_sum(double v, double* red) {
  v = tsne_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  const int nw = (int)(blockDim.x * blockDim.y) >> 6;
  for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}

// ---- squared distances ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_sqdist_kernel(const float* __restrict__ X, float* __restrict__ D2, int N,
                                                          int D) {
  __shared__ float xi[16][33], xj[16][33];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  double acc = 0.0;
  for (int d0 = 0; d0 < D; d0 += 32) {
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = d0 + tx + 16 * h;
      xi[ty][tx + 16 * h] = (i0 + ty < N && d < D) ? X[(size_t)(i0 + ty) * D + d] : 0.0f;
      xj[ty][tx + 16 * h] = (j0 + ty < N && d < D) ? X[(size_t)(j0 + ty) * D + d] : 0.0f;
    }
    __syncthreads();
    const int nd = min(32, D - d0);
    for (int d = 0; d < nd; ++d) {
      const double t = (double)xi[ty][d] - (double)xj[tx][d];
      acc += t * t;
    }
  }
  if (i0 + ty < N && j0 + tx < N) D2[(size_t)(i0 + ty) * N + j0 + tx] = (float)acc;
}

// ---- perplexity search: info (N,4) doubles = beta of the returned row, s, sum_j p_j / s, steps taken ---------------------
__global__ __launch_bounds__(256) void tsne_search_kernel(const float* __restrict__ D2, double* __restrict__ info, int N,
                                                          double log_perp) {
  __shared__ double red[16];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ row = D2 + (size_t)i * N;
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, used = 1.0, S = 1.0, RS = 0.0;
  int steps = 0;
  for (int l = 0; l < 100; ++l) {
    double s = 0.0;
    for (int j = tid; j < N; j += 256)
      if (j != i) s += exp(-(double)row[j] * beta);
    S = tsne_block_sum(s, red);
    if (S == 0.0) S = 1e-8;
    double sd = 0.0, rs = 0.0;
    for (int j = tid; j < N; j += 256)
      if (j != i) {
        const double p = exp(-(double)row[j] * beta) / S;
        sd += (double)row[j] * p;
        rs += p;
      }
    const double SD = tsne_block_sum(sd, red);
    RS = tsne_block_sum(rs, red);
    const double diff = log(S) + beta * SD - log_perp;
    used = beta;
    steps = l + 1;
    if (fabs(diff) <= 1e-5) break;      // (every thread holds the same sums: the branch is uniform)
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  if (tid == 0) {
    info[4 * (size_t)i + 0] = used;
    info[4 * (size_t)i + 1] = S;
    info[4 * (size_t)i + 2] = RS;
    info[4 * (size_t)i + 3] = (double)steps;
  }
}

__global__ __launch_bounds__(256) void tsne_psum_kernel(const double* __restrict__ info, double* __restrict__ total,
                                                        int N) {
  __shared__ double red[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) s += 2.0 * info[4 * (size_t)i + 2];
  s = tsne_block_sum(s, red);
  if (threadIdx.x == 0) total[0] = fmax(s, TSNE_EPS);
}

// P (N, ldp) fp32, ldp % 4 == 0; the columns [N, ldp) are written 0.  The pair (i, j) and the pair (j, i) run the same
// arithmetic on the same operands in the same order (the term of the smaller row index first): P is symmetric bit for bit.
__global__ __launch_bounds__(256) void tsne_joint_kernel(const float* __restrict__ D2, const double* __restrict__ info,
                                                         const double* __restrict__ total, float* __restrict__ P, int N,
                                                         int ldp) {
  const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ldp) return;
  float out = 0.0f;
  if (j < N && j != i) {
    const int a = min(i, j), b = max(i, j);
    const double d = (double)D2[(size_t)i * N + j];
    const double ca = exp(-d * info[4 * (size_t)a]) / info[4 * (size_t)a + 1];
    const double cb = exp(-d * info[4 * (size_t)b]) / info[4 * (size_t)b + 1];
    out = (float)fmax((ca + cb) / total[0], TSNE_EPS);
  }
  P[(size_t)i * ldp + j] = out;
}

// ---- one iteration, first half: the per-row sums ------------------------------------------------------------------------
// rows (N, 8) doubles.  KL: also the pieces klA = sum_j e_ij log(max(e_ij, eps) (1 + d_ij)), klB = sum_j e_ij with
// e = ex P, from which KL = klA + klB log Z once Z is known (Q_ij = w_ij / Z, w = 1 / (1 + d)); the logarithm in double,
// because the two parts cancel to a small fraction of either.
template <bool KL>
__global__ __launch_bounds__(64 * TSNE_FWAVES) void tsne_forces_kernel(const float* __restrict__ Y,
                                                                       const float* __restrict__ P,
                                                                       double* __restrict__ rows, int N, int ldp,
                                                                       double ex) {
  // every fused multiply-add of the pair terms is written out and the compiler forms none of its own, so that the two
  // instantiations round alike: the embedding does not depend on which iterations log the objective
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = (blockIdx.x * TSNE_FWAVES + wave) * TSNE_RB;
  if (i0 >= N) return;      // (wave-uniform; the kernel has no workgroup barrier)
  float yix[TSNE_RB], yiy[TSNE_RB];
  const float* prow[TSNE_RB];
  double ax[TSNE_RB], ay[TSNE_RB], rx[TSNE_RB], ry[TSNE_RB], zz[TSNE_RB], ka[TSNE_RB], kb[TSNE_RB];
#pragma unroll
  for (int r = 0; r < TSNE_RB; ++r) {
    const int ii = min(i0 + r, N - 1);      // a row past the end repeats the last one; its sums are not stored
    yix[r] = Y[2 * ii];
    yiy[r] = Y[2 * ii + 1];
    prow[r] = P + (size_t)ii * ldp;
    ax[r] = ay[r] = rx[r] = ry[r] = zz[r] = ka[r] = kb[r] = 0.0;
  }
  // the tile of the next 256 columns is fetched while the current one computes: a wave's loop is one dependent chain,
  // and at N = 10 000 a SIMD holds only two or three such waves
  f32x4 pn[TSNE_RB];
  float nyx[4], nyy[4];
  auto fetch = [&](int j) {
    if (j + 3 < N) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(Y + 2 * j), b = *reinterpret_cast<const f32x4*>(Y + 2 * j + 4);
      nyx[0] = a[0], nyy[0] = a[1], nyx[1] = a[2], nyy[1] = a[3];
      nyx[2] = b[0], nyy[2] = b[1], nyx[3] = b[2], nyy[3] = b[3];
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int jj = min(j + v, N - 1);
        nyx[v] = Y[2 * jj];
        nyy[v] = Y[2 * jj + 1];
      }
    }
#pragma unroll
    for (int r = 0; r < TSNE_RB; ++r) pn[r] = *reinterpret_cast<const f32x4*>(prow[r] + j);
  };
  if (4 * lane < ldp) fetch(4 * lane);
  for (int j0 = 0; j0 < ldp; j0 += 256) {
    const int j = j0 + 4 * lane;            // ldp % 4 == 0: a lane's four columns are inside the padded row or all outside
    if (j >= ldp) continue;
    f32x4 pc[TSNE_RB];
    float yjx[4], yjy[4];
#pragma unroll
    for (int r = 0; r < TSNE_RB; ++r) pc[r] = pn[r];
#pragma unroll
    for (int v = 0; v < 4; ++v) yjx[v] = nyx[v], yjy[v] = nyy[v];
    if (j + 256 < ldp) fetch(j + 256);
#pragma unroll
    for (int r = 0; r < TSNE_RB; ++r) {
      const f32x4 p4 = pc[r];
      float fax = 0.f, fay = 0.f, frx = 0.f, fry = 0.f, fz = 0.f;
      double fka = 0.0, fkb = 0.0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const bool on = (j + v < N) && (j + v != i0 + r);
        const float dx = yix[r] - yjx[v], dy = yiy[r] - yjy[v];
        const float d2 = fmaf(dx, dx, dy * dy);
        const float w = on ? 1.0f / (1.0f + d2) : 0.0f;
        const float p = on ? p4[v] : 0.0f;
        const float pw = p * w, w2 = w * w;
        fax = fmaf(pw, dx, fax);
        fay = fmaf(pw, dy, fay);
        frx = fmaf(w2, dx, frx);
        fry = fmaf(w2, dy, fry);
        fz += w;
        if (KL) {
          if (on) {
            const double e = ex * (double)p;
            fka += e * log(fmax(e, TSNE_EPS) * (1.0 + (double)d2));
            fkb += e;
          }
        }
      }
      ax[r] += (double)fax;
      ay[r] += (double)fay;
      rx[r] += (double)frx;
      ry[r] += (double)fry;
      zz[r] += (double)fz;
      if (KL) {
        ka[r] += fka;
        kb[r] += fkb;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < TSNE_RB; ++r) {
    const double s0 = tsne_wave_sum(ax[r]), s1 = tsne_wave_sum(ay[r]), s2 = tsne_wave_sum(rx[r]);
    const double s3 = tsne_wave_sum(ry[r]), s4 = tsne_wave_sum(zz[r]);
    const double s5 = KL ? tsne_wave_sum(ka[r]) : 0.0, s6 = KL ? tsne_wave_sum(kb[r]) : 0.0;
    if (lane == 0 && i0 + r < N) {
      double* o = rows + (size_t)(i0 + r) * TSNE_ROW_DOUBLES;
      o[0] = s0;
      o[1] = s1;
      o[2] = s2;
      o[3] = s3;
      o[4] = s4;
      o[5] = s5;
      o[6] = s6;
      o[7] = 0.0;
    }
  }
}

// ---- one iteration, second half ------------------------------------------------------------------------------------------
// state (3, N, 2) fp32 = Y | upd | gains.  apply: the gains / momentum update in place and log2 = (KL, |g|) of this
// iteration; else (mmvae_tsne_forces) g (N,2) fp32 and kz = (KL, Z), the state untouched.  KL is NaN unless has_kl.
__global__ __launch_bounds__(TSNE_UPD_THREADS) void tsne_update_kernel(float* __restrict__ state,
                                                                       const double* __restrict__ rows, int N, double ex,
                                                                       double mom, double lr, int has_kl, int apply,
                                                                       double* __restrict__ log2, float* __restrict__ g,
                                                                       double* __restrict__ kz) {
  __shared__ double red[16];
  const int tid = threadIdx.x;
  double z = 0.0, ka = 0.0, kb = 0.0;
  for (int i = tid; i < N; i += TSNE_UPD_THREADS) {
    const double* r = rows + (size_t)i * TSNE_ROW_DOUBLES;
    z += r[4];
    ka += r[5];
    kb += r[6];
  }
  const double Z = tsne_block_sum(z, red);
  const double KA = tsne_block_sum(ka, red), KB = tsne_block_sum(kb, red);
  float* __restrict__ Y = state;
  float* __restrict__ U = state + 2 * (size_t)N;
  float* __restrict__ G = state + 4 * (size_t)N;
  double n2 = 0.0;
  for (int e = tid; e < 2 * N; e += TSNE_UPD_THREADS) {
    const double* r = rows + (size_t)(e >> 1) * TSNE_ROW_DOUBLES;
    const double gr = 4.0 * (ex * r[e & 1] - r[2 + (e & 1)] / Z);
    n2 += gr * gr;
    if (apply) {
      const double u = (double)U[e];
      double ga = (double)G[e];
      ga = (u * gr < 0.0) ? ga + 0.2 : ga * 0.8;
      ga = fmax(ga, 0.01);
      const double un = mom * u - lr * (ga * gr);
      G[e] = (float)ga;
      U[e] = (float)un;
      Y[e] = (float)((double)Y[e] + (double)(float)un);
    } else {
      g[e] = (float)gr;
    }
  }
  const double N2 = tsne_block_sum(n2, red);
  if (tid == 0) {
    const double kl = has_kl ? KA + KB * log(Z) : (double)NAN;
    if (apply) {
      log2[0] = kl;
      log2[1] = sqrt(N2);
    } else {
      kz[0] = kl;
      kz[1] = Z;
    }
  }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
static bool tsne_n_ok(int N) { return N >= MMVAE_TSNE_MIN_POINTS && N <= MMVAE_TSNE_MAX_POINTS; }

extern "C" int mmvae_tsne_ld(int N) { return tsne_n_ok(N) ? (N + 3) & ~3 : 0; }

extern "C" int mmvae_tsne_sqdist(const float* X, float* D2, int N, int D, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(X && D2 && N > 0 && D > 0);
  if (!tsne_n_ok(N) || D > MMVAE_TSNE_MAX_DIM) return MMVAE_ERR_UNSUPPORTED;
  const int t = (N + 15) / 16;
  hipLaunchKernelGGL(tsne_sqdist_kernel, dim3(t, t), dim3(256), 0, (hipStream_t)stream, X, D2, N, D);
  return mmvae_launch_status();
}

extern "C" int mmvae_tsne_joint_p(const float* D2, double perplexity, float* P, int ldp, double* info, double* total,
                                  int N, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(D2 && P && info && total && N > 0 && perplexity > 0.0);
  if (!tsne_n_ok(N) || ldp != mmvae_tsne_ld(N)) return MMVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(tsne_search_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, D2, info, N, log(perplexity));
  hipLaunchKernelGGL(tsne_psum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, info, total, N);
  hipLaunchKernelGGL(tsne_joint_kernel, dim3((ldp + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, D2, info, total, P,
                     N, ldp);
  return mmvae_launch_status();
}

static void tsne_launch_forces(const float* Y, const float* P, double* rows, int N, int ldp, double ex, bool kl,
                               hipStream_t s) {
  const int grid = (N + TSNE_FWAVES * TSNE_RB - 1) / (TSNE_FWAVES * TSNE_RB);
  if (kl)
    hipLaunchKernelGGL(tsne_forces_kernel<true>, dim3(grid), dim3(64 * TSNE_FWAVES), 0, s, Y, P, rows, N, ldp, ex);
  else
    hipLaunchKernelGGL(tsne_forces_kernel<false>, dim3(grid), dim3(64 * TSNE_FWAVES), 0, s, Y, P, rows, N, ldp, ex);
}

extern "C" size_t mmvae_tsne_ws_doubles(int N) { return tsne_n_ok(N) ? (size_t)N * TSNE_ROW_DOUBLES : 0; }

extern "C" int mmvae_tsne_forces(const float* state, const float* P, int ldp, double* ws, float* g, double* kz, int N,
                                 long it, long switch_it, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && P && ws && g && kz && N > 0 && it >= 0);
  if (!tsne_n_ok(N) || ldp != mmvae_tsne_ld(N)) return MMVAE_ERR_UNSUPPORTED;
  const double ex = it < switch_it ? 12.0 : 1.0;
  tsne_launch_forces(state, P, ws, N, ldp, ex, true, (hipStream_t)stream);
  hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(TSNE_UPD_THREADS), 0, (hipStream_t)stream,
                     const_cast<float*>(state), ws, N, ex, 0.0, 0.0, 1, 0, (double*)nullptr, g, kz);
  return mmvae_launch_status();
}

extern "C" int mmvae_tsne_run(float* state, const float* P, int ldp, double* ws, double* log, int N, long it0, int n_iter,
                              long switch_it, double lr, int kl_every, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && P && ws && log && N > 0 && it0 >= 0 && n_iter > 0 && lr > 0.0 && kl_every > 0);
  if (!tsne_n_ok(N) || ldp != mmvae_tsne_ld(N)) return MMVAE_ERR_UNSUPPORTED;
  for (int k = 0; k < n_iter; ++k) {
    const long it = it0 + k;
    const bool early = it < switch_it;
    const double ex = early ? 12.0 : 1.0;
    const bool kl = (it + 1) % kl_every == 0;      // (a function of `it` alone: a split run logs the same rows)
    tsne_launch_forces(state, P, ws, N, ldp, ex, kl, (hipStream_t)stream);
    hipLaunchKernelGGL(tsne_update_kernel, dim3(1), dim3(TSNE_UPD_THREADS), 0, (hipStream_t)stream, state, ws, N, ex,
                       early ? 0.5 : 0.8, lr, kl ? 1 : 0, 1, log + 2 * (size_t)k, (float*)nullptr, (double*)nullptr);
  }
  return mmvae_launch_status();
}
