// Frechet distance of generated images (TorchMMVAE.frechet_distances): the arithmetic of the reference's
// calculate_frechet_distance (eval/fid_score.py), d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2, all in double.
//   fr_colmean_kernel    batch mean of X (n_b, F) fp32, rows summed in double in a fixed order
//   f64_tile_kernel      ONE fp64 MFMA tile routine (f64_tile.hpp, shared with cca.hip; v_mfma_f64_16x16x4_f64; 64 x 64 tile
//                        per workgroup, 32 x 32 per wave)
//                        behind three products: the centred scatter of a batch merged into M2 by Chan's rule (SYRK, upper
//                        tiles computed, mirrored on the store), C = A B and C = A B^T
//   fr_merge_mean_kernel mean += delta n_b / (n + n_b), n += n_b
//   eig_*                one-sided (Hestenes) Jacobi in round-robin order: one launch per step, one wave (F <= 256) or one
//                        workgroup of four waves (F > 256) per pair; pairs of a step share no column, so a launch needs no
//                        communication between workgroups
//   fr_distance_kernel   the traces and the final sum, one workgroup, fixed order
// No atomics; every sum has one owner and one order: two runs give the same bits.
#include "f64_tile.hpp"

#define EIG_TAU2 1e-30        // tau^2, tau = 1e-15: rotate when c^2 > tau^2 a b
#define EIG_WIDE_F 256        // above: four waves per pair

static bool fr_f_ok(int F) { return F >= 1 && F <= MMVAE_FRECHET_MAX_F; }

__device__ __forceinline__ double fr_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- batch mean ----------------------------------------------------------------------------------------------------------
// grid ceil(F / 64), 256 threads: lane = column, wave w sums the rows [w R, (w + 1) R), R = ceil(nb / 4), in row order;
// the four partials are added as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(256) void fr_colmean_kernel(const float* __restrict__ X, double* __restrict__ mean_b, long nb,
                                                         int F) {
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = blockIdx.x * 64 + lane;
  const long R = (nb + 3) >> 2, r0 = wave * R, r1 = min(nb, r0 + R);
  double s = 0.0;
  if (j < F)
    for (long r = r0; r < r1; ++r) s += (double)X[(size_t)r * F + j];
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && j < F) mean_b[j] = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) / (double)nb;
}

// ---- the fp64 MFMA tile routine (f64_tile.hpp): the operands and stores of this file --------------------------------------
struct FrSyrkOp {      // the centred batch: element (i, k) = (double)X[k][i] - mean_b[i]
  const float* X;
  const double* mean_b;
  long nb;
  int F;
  static constexpr bool KFAST = false;
  __device__ __forceinline__ double operator()(int i, long k) const {
    return (i < F && k < nb) ? (double)X[(size_t)k * F + i] - mean_b[i] : 0.0;
  }
};
struct FrRowOp {       // element (i, k) = M[i][k]
  const double* M;
  int F;
  static constexpr bool KFAST = true;
  __device__ __forceinline__ double operator()(int i, long k) const { return (i < F && k < F) ? M[(size_t)i * F + k] : 0.0; }
};
struct FrColOp {       // element (i, k) = M[k][i]
  const double* M;
  int F;
  static constexpr bool KFAST = false;
  __device__ __forceinline__ double operator()(int i, long k) const { return (i < F && k < F) ? M[(size_t)k * F + i] : 0.0; }
};
struct FrStore {       // C[i][j] = v
  double* C;
  int F;
  static constexpr bool UPPER = false;
  __device__ __forceinline__ void operator()(int i, int j, double v) const { C[(size_t)i * F + j] = v; }
};
struct FrChanStore {   // M2[i][j] += v + delta_i delta_j n n_b / (n + n_b), the tile below the diagonal written as the mirror
  double* state;       // n | mean (F) | M2 (F, F)
  const double* mean_b;
  long nb;
  int F;
  static constexpr bool UPPER = true;
  __device__ __forceinline__ void operator()(int i, int j, double v) const {
    const double n = state[0], w = n * (double)nb / (n + (double)nb);
    const double di = mean_b[i] - state[1 + i], dj = mean_b[j] - state[1 + j];
    double* M2 = state + 1 + F;
    const double out = M2[(size_t)i * F + j] + (v + (di * dj) * w);
    M2[(size_t)i * F + j] = out;
    if ((i / FR_TILE) != (j / FR_TILE)) M2[(size_t)j * F + i] = out;
  }
};

template <class OpA, class OpB, class Store>
static void fr_launch_tiles(OpA a, OpB b, Store st, int M, long K, hipStream_t s) {
  f64_launch_tiles(a, b, st, M, M, K, s);
}

// ---- moments ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fr_merge_mean_kernel(double* __restrict__ state, const double* __restrict__ mean_b,
                                                            long nb, int F) {
  // one workgroup: every thread reads n before the barrier, thread 0 writes it after
  const double n = state[0], tot = n + (double)nb;
  for (int j = threadIdx.x; j < F; j += 256) state[1 + j] += (mean_b[j] - state[1 + j]) * ((double)nb / tot);
  __syncthreads();
  if (threadIdx.x == 0) state[0] = tot;
}

__global__ __launch_bounds__(256) void fr_finish_kernel(const double* __restrict__ state, double* __restrict__ mu,
                                                        double* __restrict__ sigma, int F) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, FF = (size_t)F * F;
  const double dof = state[0] - 1.0;
  if (e < FF) sigma[e] = state[1 + F + e] / dof;
  if (e < (size_t)F) mu[e] = state[1 + e];
}

extern "C" size_t mmvae_frechet_state_doubles(int F) { return fr_f_ok(F) ? 1 + (size_t)F + (size_t)F * F : 0; }

extern "C" int mmvae_frechet_update(double* state, const float* X, double* ws, long nb, int F, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && X && ws && nb > 0);
  if (!fr_f_ok(F)) return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fr_colmean_kernel, dim3((F + 63) / 64), dim3(256), 0, s, X, ws, nb, F);
  const FrSyrkOp op = {X, ws, nb, F};
  fr_launch_tiles(op, op, FrChanStore{state, ws, nb, F}, F, nb, s);
  hipLaunchKernelGGL(fr_merge_mean_kernel, dim3(1), dim3(256), 0, s, state, ws, nb, F);
  return mmvae_launch_status();
}

extern "C" int mmvae_frechet_finish(const double* state, double* mu, double* sigma, long n, int F, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && mu && sigma);
  if (!fr_f_ok(F) || n < 2) return MMVAE_ERR_UNSUPPORTED;
  const size_t FF = (size_t)F * F;
  hipLaunchKernelGGL(fr_finish_kernel, dim3((unsigned)((FF + 255) / 256)), dim3(256), 0, (hipStream_t)stream, state, mu,
                     sigma, F);
  return mmvae_launch_status();
}

extern "C" int mmvae_f64_gemm(const double* A, const double* B, double* C, int F, int trans_b, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(A && B && C && C != A && C != B);
  if (!fr_f_ok(F)) return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  // the B operand functor is asked for (j, k): B[k][j] for A B, B[j][k] for A B^T
  if (trans_b)
    fr_launch_tiles(FrRowOp{A, F}, FrRowOp{B, F}, FrStore{C, F}, F, (long)F, s);
  else
    fr_launch_tiles(FrRowOp{A, F}, FrColOp{B, F}, FrStore{C, F}, F, (long)F, s);
  return mmvae_launch_status();
}

// ---- symmetric eigensolver: one-sided Jacobi ---------------------------------------------------------------------------------
// A (F, F): column j is the F doubles at A + j F (for a symmetric input the row-major matrix is that layout); Vc likewise:
// Vc[j F + i] = V[i][j].  misc: [0] floor^2, ints from misc + 8: flags (n / 2) | counts (MMVAE_EIG_MAX_SWEEPS).
__global__ __launch_bounds__(256) void eig_colnorm_kernel(const double* __restrict__ A, double* __restrict__ out, int F,
                                                          int root) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= F) return;      // (wave-uniform; no barrier)
  const double* __restrict__ c = A + (size_t)j * F;
  double s = 0.0;
  for (int i = lane; i < F; i += 64) s += c[i] * c[i];
  s = fr_wave_sum(s);
  if (lane == 0) out[j] = root ? sqrt(s) : s;
}

// floor^2 = (F 2^-52 max_j |S_j|)^2 from the squared column norms; also clears the flags
__global__ __launch_bounds__(256) void eig_floor_kernel(const double* __restrict__ norm2, double* __restrict__ misc, int F,
                                                        int half) {
  __shared__ double red[256];
  double m = 0.0;
  for (int j = threadIdx.x; j < F; j += 256) m = fmax(m, norm2[j]);
  red[threadIdx.x] = m;
  __syncthreads();
  int* ints = reinterpret_cast<int*>(misc + 8);
  for (int k = threadIdx.x; k < half + MMVAE_EIG_MAX_SWEEPS; k += 256) ints[k] = 0;
  if (threadIdx.x == 0) {
    for (int t = 1; t < 256; ++t) m = fmax(m, red[t]);
    const double f = (double)F * 2.220446049250313e-16;
    misc[0] = (f * f) * m;
  }
}

__global__ __launch_bounds__(256) void eig_identity_kernel(double* __restrict__ Vc, int F) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (size_t)F * F) Vc[e] = (e / F == e % F) ? 1.0 : 0.0;
}

// One step of the round-robin ordering over n = F + (F odd) columns: pair k of step s is (n - 1, s) for k = 0 and
// ((s + k) mod (n - 1), (s - k) mod (n - 1)) for k >= 1; a pair that touches the padding column F is skipped.
// WPP waves per pair, 256 threads: 4 / WPP pairs per workgroup.  EPT = elements of a column per thread (registers).
template <int WPP, int EPT>
__global__ __launch_bounds__(256) void eig_step_kernel(double* __restrict__ A, double* __restrict__ Vc,
                                                       double* __restrict__ misc, int F, int n, int step) {
  __shared__ double red[3][4];
  constexpr int T = 64 * WPP;
  const int tid = threadIdx.x % T, k = blockIdx.x * (4 / WPP) + threadIdx.x / T;
  if (k >= n / 2) return;      // (uniform over the threads of a pair; WPP = 4: over the workgroup)
  int p, q;
  if (k == 0) {
    p = n - 1;
    q = step;
  } else {
    p = (step + k) % (n - 1);
    q = (step - k + (n - 1)) % (n - 1);
  }
  if (p > q) {
    const int t = p;
    p = q;
    q = t;
  }
  if (q >= F) return;          // the padding column
  double* __restrict__ cp = A + (size_t)p * F;
  double* __restrict__ cq = A + (size_t)q * F;
  double xp[EPT], xq[EPT];
  double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * T;
    xp[e] = i < F ? cp[i] : 0.0;
    xq[e] = i < F ? cq[i] : 0.0;
    a += xp[e] * xp[e];
    b += xq[e] * xq[e];
    c += xp[e] * xq[e];
  }
  // the butterfly leaves the same bits in every lane (each level adds the same two values in either order)
  a = fr_wave_sum(a);
  b = fr_wave_sum(b);
  c = fr_wave_sum(c);
  if (WPP > 1) {
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = a;
      red[1][threadIdx.x >> 6] = b;
      red[2][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    c = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
  }
  if (!(c != 0.0 && c * c > EIG_TAU2 * a * b)) return;      // (NaN input: never rotates)
  const double zeta = (b - a) / (2.0 * c);
  // |zeta| = inf (c tiny): the quotient is 0, the right limit; zeta is never NaN here (c != 0, a and b finite)
  double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  if (zeta < 0.0) t = -t;
  const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * T;
    if (i < F) {
      cp[i] = cs * xp[e] - sn * xq[e];
      cq[i] = sn * xp[e] + cs * xq[e];
    }
  }
  if (Vc) {
    double* __restrict__ vp = Vc + (size_t)p * F;
    double* __restrict__ vq = Vc + (size_t)q * F;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int i = tid + e * T;
      if (i < F) {
        const double u = vp[i], w = vq[i];
        vp[i] = cs * u - sn * w;
        vq[i] = sn * u + cs * w;
      }
    }
  }
  // counted towards convergence only when both columns stand above the floor; slot k has one writer per launch
  if (tid == 0 && a > misc[0] && b > misc[0]) {
    int* flags = reinterpret_cast<int*>(misc + 8);
    flags[k] = flags[k] + 1;
  }
}

// end of a sweep: counts[sweep] = sum of the flags, which are cleared for the next sweep
__global__ __launch_bounds__(256) void eig_count_kernel(double* __restrict__ misc, int half, int sweep) {
  __shared__ int red[256];
  int* flags = reinterpret_cast<int*>(misc + 8);
  int s = 0;
  for (int k = threadIdx.x; k < half; k += 256) {
    s += flags[k];
    flags[k] = 0;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < 256; ++t) s += red[t];
    flags[half + sweep] = s;
  }
}

extern "C" size_t mmvae_sym_eig_ws_doubles(int F) { return fr_f_ok(F) ? (size_t)F * F + 2 * (size_t)F + 64 : 0; }

extern "C" int mmvae_sym_eig_waves_per_pair(int F) { return !fr_f_ok(F) ? 0 : F <= EIG_WIDE_F ? 1 : 4; }

// ws: A (F F) | norms (F) | misc (F + 64).  S == ws is allowed (the matrix is already in place and is destroyed).
static int eig_run(const double* S, double* ws, double* Vc, double* values, int* sweeps, int* rotations, int F,
                   int max_sweeps, hipStream_t s) {
  double* A = ws;
  double* norms = ws + (size_t)F * F;
  double* misc = norms + F;
  const int n = F + (F & 1), half = n / 2;
  const size_t FF = (size_t)F * F;
  if (S != A && hipMemcpyAsync(A, S, FF * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) return MMVAE_ERR_LAUNCH;
  if (Vc) hipLaunchKernelGGL(eig_identity_kernel, dim3((unsigned)((FF + 255) / 256)), dim3(256), 0, s, Vc, F);
  hipLaunchKernelGGL(eig_colnorm_kernel, dim3((F + 3) / 4), dim3(256), 0, s, A, norms, F, 0);
  hipLaunchKernelGGL(eig_floor_kernel, dim3(1), dim3(256), 0, s, norms, misc, F, half);
  const int* counts = reinterpret_cast<const int*>(misc + 8) + half;
  int done = 0, rc = MMVAE_ERR_NO_CONVERGENCE;
  for (int sw = 0; sw < max_sweeps; ++sw) {
    for (int step = 0; step < n - 1; ++step) {
      if (F <= EIG_WIDE_F)
        hipLaunchKernelGGL((eig_step_kernel<1, EIG_WIDE_F / 64>), dim3((half + 3) / 4), dim3(256), 0, s, A, Vc, misc, F, n,
                           step);
      else
        hipLaunchKernelGGL((eig_step_kernel<4, MMVAE_FRECHET_MAX_F / 256>), dim3(half), dim3(256), 0, s, A, Vc, misc, F, n,
                           step);
    }
    hipLaunchKernelGGL(eig_count_kernel, dim3(1), dim3(256), 0, s, misc, half, sw);
    int counted = 0;      // the one integer the host reads per sweep
    if (hipMemcpyAsync(&counted, counts + sw, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return MMVAE_ERR_LAUNCH;
    rotations[sw] = counted;
    done = sw + 1;
    if (counted == 0) {
      rc = MMVAE_OK;
      break;
    }
  }
  *sweeps = done;
  hipLaunchKernelGGL(eig_colnorm_kernel, dim3((F + 3) / 4), dim3(256), 0, s, A, values, F, 1);
  const int st = mmvae_launch_status();
  return st != MMVAE_OK ? st : rc;
}

extern "C" int mmvae_sym_eig(const double* S, double* ws, double* Vc, double* values, int* sweeps, int* rotations, int F,
                             int max_sweeps, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(S && ws && values && sweeps && rotations && S != ws);
  if (!fr_f_ok(F) || max_sweeps < 1 || max_sweeps > MMVAE_EIG_MAX_SWEEPS) return MMVAE_ERR_UNSUPPORTED;
  return eig_run(S, ws, Vc, values, sweeps, rotations, F, max_sweeps, (hipStream_t)stream);
}

// ---- the distance ----------------------------------------------------------------------------------------------------------
// R = diag(sqrt(lambda)) V^T: row j of the column-contiguous V scaled in place
__global__ __launch_bounds__(256) void fr_scale_rows_kernel(double* __restrict__ Vc, const double* __restrict__ lam, int F) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (size_t)F * F) Vc[e] *= sqrt(lam[e / F]);
}

// out = (d^2, tr covmean, |mu1 - mu2|^2, tr S1, tr S2): thread t sums the elements t, t + 256, ... in order, the 256
// partials are added in thread order
__global__ __launch_bounds__(256) void fr_distance_kernel(const double* __restrict__ mu1, const double* __restrict__ s1,
                                                          const double* __restrict__ mu2, const double* __restrict__ s2,
                                                          const double* __restrict__ sv, double* __restrict__ out, int F) {
  __shared__ double red[4][256];
  double d = 0.0, t1 = 0.0, t2 = 0.0, tc = 0.0;
  for (int j = threadIdx.x; j < F; j += 256) {
    const double u = mu1[j] - mu2[j];
    d += u * u;
    t1 += s1[(size_t)j * F + j];
    t2 += s2[(size_t)j * F + j];
    tc += sqrt(sv[j]);
  }
  red[0][threadIdx.x] = d;
  red[1][threadIdx.x] = t1;
  red[2][threadIdx.x] = t2;
  red[3][threadIdx.x] = tc;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < 256; ++t) {
      d += red[0][t];
      t1 += red[1][t];
      t2 += red[2][t];
      tc += red[3][t];
    }
    out[0] = d + t1 + t2 - 2.0 * tc;
    out[1] = tc;
    out[2] = d;
    out[3] = t1;
    out[4] = t2;
  }
}

extern "C" size_t mmvae_frechet_ws_doubles(int F) {
  return fr_f_ok(F) ? mmvae_sym_eig_ws_doubles(F) + 2 * (size_t)F * F + 2 * (size_t)F : 0;
}

// ws: eigensolver workspace | Vc -> R (F F) | T (F F) | lambda (F) | sigma(G) (F)
extern "C" int mmvae_frechet_distance(const double* mu1, const double* sigma1, const double* mu2, const double* sigma2,
                                      double* ws, double* out, int* sweeps, int F, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(mu1 && sigma1 && mu2 && sigma2 && ws && out && sweeps);
  if (!fr_f_ok(F)) return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const size_t FF = (size_t)F * F;
  double* eig = ws;
  double* R = ws + mmvae_sym_eig_ws_doubles(F);
  double* T = R + FF;
  double* lam = T + FF;
  double* sv = lam + F;
  int rot[MMVAE_EIG_MAX_SWEEPS];
  sweeps[0] = sweeps[1] = 0;
  int rc = eig_run(sigma1, eig, R, lam, &sweeps[0], rot, F, MMVAE_EIG_MAX_SWEEPS, s);
  if (rc != MMVAE_OK) return rc;
  hipLaunchKernelGGL(fr_scale_rows_kernel, dim3((unsigned)((FF + 255) / 256)), dim3(256), 0, s, R, lam, F);
  fr_launch_tiles(FrRowOp{sigma2, F}, FrRowOp{R, F}, FrStore{T, F}, F, (long)F, s);      // T = S2 R^T
  fr_launch_tiles(FrRowOp{R, F}, FrColOp{T, F}, FrStore{eig, F}, F, (long)F, s);         // G = R T, in the solver's place
  rc = eig_run(eig, eig, nullptr, sv, &sweeps[1], rot, F, MMVAE_EIG_MAX_SWEEPS, s);
  if (rc != MMVAE_OK) return rc;
  hipLaunchKernelGGL(fr_distance_kernel, dim3(1), dim3(256), 0, s, mu1, sigma1, mu2, sigma2, sv, out, F);
  return mmvae_launch_status();
}
