// Cross-modal correlation of generations (TorchMMVAE.cross_modal_correlation): the arithmetic of the reference's cca /
// apply_weights / apply_pc (eval/mnistsvhn_helper.py), all in double.
//   mmvae_f64_gemm_ld        the fp64 MFMA tile routine of f64_tile.hpp on sub-blocks: C (M, N) = (A diag(scale)) B or
//                            (A diag(scale)) B^T with leading dimensions, M, N, K no multiples of the tile (ops.cca_fit:
//                            Q L^-1/2 Q^T and W_i sigma_ij W_j in place in the (O, O) matrices)
//   cca_score_kernel         per row r: p = (a_r - mean_a) P_a, q = (b_r - mean_b) P_b on the fp64 MFMA (64 rows x all
//                            k <= 64 columns of both views per workgroup), cos_r = p . q / (max(|p|, 1e-8) max(|q|, 1e-8));
//                            the projections are never written
//   cca_sum_kernel           the sum of the rows' cosines, one workgroup, fixed order
//   sentence_kernel          one wave per sentence: the weighted mean of the embeddings up to the first eos, minus its
//                            component along pc, in double in token order, one rounding to fp32
// No atomics; every sum has one owner and one order: two runs give the same bits.
#include "f64_tile.hpp"

static bool cca_dim_ok(int n) { return n >= 1 && n <= MMVAE_FRECHET_MAX_F; }

// ---- C = (A diag(scale)) op(B) on sub-blocks ---------------------------------------------------------------------------------
struct CcaAOp {        // element (i, k) = A[i][k] (scale[k])
  const double* A;
  const double* scale;
  int lda, M, K;
  static constexpr bool KFAST = true;
  __device__ __forceinline__ double operator()(int i, long k) const {
    if (!(i < M && k < K)) return 0.0;
    const double v = A[(size_t)i * lda + k];
    return scale ? v * scale[k] : v;
  }
};
struct CcaBRowOp {     // B (N, K): element (j, k) = B[j][k]
  const double* B;
  int ldb, N, K;
  static constexpr bool KFAST = true;
  __device__ __forceinline__ double operator()(int j, long k) const { return (j < N && k < K) ? B[(size_t)j * ldb + k] : 0.0; }
};
struct CcaBColOp {     // B (K, N): element (j, k) = B[k][j]
  const double* B;
  int ldb, N, K;
  static constexpr bool KFAST = false;
  __device__ __forceinline__ double operator()(int j, long k) const { return (j < N && k < K) ? B[(size_t)k * ldb + j] : 0.0; }
};
struct CcaStore {      // C[i][j] = v
  double* C;
  int ldc;
  static constexpr bool UPPER = false;
  __device__ __forceinline__ void operator()(int i, int j, double v) const { C[(size_t)i * ldc + j] = v; }
};

extern "C" int mmvae_f64_gemm_ld(const double* A, int lda, const double* B, int ldb, double* C, int ldc, const double* scale,
                                 int M, int N, int K, int trans_b, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(A && B && C && C != A && C != B);
  if (!cca_dim_ok(M) || !cca_dim_ok(N) || !cca_dim_ok(K)) return MMVAE_ERR_UNSUPPORTED;
  if (lda < K || ldb < (trans_b ? K : N) || ldc < N) return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const CcaAOp a = {A, scale, lda, M, K};
  if (trans_b)
    f64_launch_tiles(a, CcaBRowOp{B, ldb, N, K}, CcaStore{C, ldc}, M, N, (long)K, s);
  else
    f64_launch_tiles(a, CcaBColOp{B, ldb, N, K}, CcaStore{C, ldc}, M, N, (long)K, s);
  return mmvae_launch_status();
}

// ---- the score ---------------------------------------------------------------------------------------------------------------
// one product of the tile: acc += (X[r0 .., :] - mean) P over the o features, k-depth FR_KT per stage; the P tile is padded
// with zero columns to 64.  A thread's eight elements of the next stage are fetched while this stage's MFMAs run.
struct CcaStage {
  double a[FR_TILE * FR_KT / 256], b[FR_TILE * FR_KT / 256];
};

__device__ __forceinline__ void cca_fetch(CcaStage& st, const float* __restrict__ X, const double* __restrict__ mean,
                                          const double* __restrict__ P, long rows, long r0, int o, int k, int k0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < FR_TILE * FR_KT / 256; ++e) {
    const int idx = tid + 256 * e;
    const int ia = idx >> 4, ka = idx & 15;          // the feature is the contiguous index of a row
    const long r = r0 + ia;
    st.a[e] = (r < rows && k0 + ka < o) ? (double)X[(size_t)r * o + k0 + ka] - mean[k0 + ka] : 0.0;
    const int jb = idx & 63, kb = idx >> 6;          // the column is the contiguous index of P
    st.b[e] = (jb < k && k0 + kb < o) ? P[(size_t)(k0 + kb) * k + jb] : 0.0;
  }
}

__device__ __forceinline__ void cca_project(const float* __restrict__ X, const double* __restrict__ mean,
                                            const double* __restrict__ P, long rows, long r0, int o, int k,
                                            double (*As)[FR_LD], double (*Bs)[FR_LD], f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, lr = lane & 15, lk = lane >> 4;
  CcaStage st;
  cca_fetch(st, X, mean, P, rows, r0, o, k, 0);
  for (int k0 = 0; k0 < o; k0 += FR_KT) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < FR_TILE * FR_KT / 256; ++e) {
      const int idx = tid + 256 * e;
      As[idx & 15][idx >> 4] = st.a[e];
      Bs[idx >> 6][idx & 63] = st.b[e];
    }
    __syncthreads();
    if (k0 + FR_KT < o) cca_fetch(st, X, mean, P, rows, r0, o, k, k0 + FR_KT);      // (workgroup-uniform)
    f64_mfma_slab<FR_KT, FR_LD, FR_KT / 4>(As, Bs, wm, wn, lr, lk, acc);
  }
}

// the sum over the 16 lanes that hold one row's 16 columns (the butterfly leaves the same bits in each of them)
__device__ __forceinline__ double cca_sum16(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid ceil(rows / 64), 256 threads; wave w holds rows [32 (w >> 1), + 32) x columns [32 (w & 1), + 32) of both products
__global__ __launch_bounds__(256) void cca_score_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const double* __restrict__ mean_a, const double* __restrict__ mean_b,
                                                        const double* __restrict__ Pa, const double* __restrict__ Pb,
                                                        double* __restrict__ cosv, long rows, int oa, int ob, int k) {
  __shared__ double As[FR_KT][FR_LD], Bs[FR_KT][FR_LD];
  __shared__ double red[3][2][FR_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, half = wave & 1, lr = lane & 15, lk = lane >> 4;
  const long r0 = (long)blockIdx.x * FR_TILE;
  f64x4 p[2][2], q[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) p[mi][ni] = q[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
  cca_project(a, mean_a, Pa, rows, r0, oa, k, As, Bs, p);
  cca_project(b, mean_b, Pb, rows, r0, ob, k, As, Bs, q);
  // a lane holds row 16 mi + lk + 4 r of its wave's 32, columns lr and 16 + lr: the two columns in order, then the 16 lanes,
  // then the two waves of a row
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double pq = cca_sum16(p[mi][0][r] * q[mi][0][r] + p[mi][1][r] * q[mi][1][r]);
      const double pp = cca_sum16(p[mi][0][r] * p[mi][0][r] + p[mi][1][r] * p[mi][1][r]);
      const double qq = cca_sum16(q[mi][0][r] * q[mi][0][r] + q[mi][1][r] * q[mi][1][r]);
      if (lr == 0) {
        const int row = wm + 16 * mi + lk + 4 * r;
        red[0][half][row] = pq;
        red[1][half][row] = pp;
        red[2][half][row] = qq;
      }
    }
  __syncthreads();
  if (tid < FR_TILE && r0 + tid < rows) {
    const double pq = red[0][0][tid] + red[0][1][tid];
    const double np = sqrt(red[1][0][tid] + red[1][1][tid]), nq = sqrt(red[2][0][tid] + red[2][1][tid]);
    cosv[r0 + tid] = pq / (fmax(np, 1e-8) * fmax(nq, 1e-8));      // F.cosine_similarity's clamp
  }
}

// thread t of 256 sums the rows t, t + 256, ... in order, the partials are added in thread order
__global__ __launch_bounds__(256) void cca_sum_kernel(const double* __restrict__ cosv, double* __restrict__ sum, long rows) {
  __shared__ double red[256];
  double s = 0.0;
  for (long r = threadIdx.x; r < rows; r += 256) s += cosv[r];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < 256; ++t) s += red[t];
    sum[0] = s;
  }
}

extern "C" int mmvae_cca_score(const float* a, const float* b, const double* mean_a, const double* mean_b, const double* proj_a,
                               const double* proj_b, double* cosv, double* sum, long rows, int oa, int ob, int k,
                               mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(a && b && mean_a && mean_b && proj_a && proj_b && cosv && sum);
  if (rows < 1 || rows > MMVAE_CCA_MAX_ROWS || !cca_dim_ok(oa) || !cca_dim_ok(ob) || k < 1 || k > MMVAE_CCA_MAX_K)
    return MMVAE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cca_score_kernel, dim3((unsigned)((rows + FR_TILE - 1) / FR_TILE)), dim3(256), 0, s, a, b, mean_a, mean_b,
                     proj_a, proj_b, cosv, rows, oa, ob, k);
  hipLaunchKernelGGL(cca_sum_kernel, dim3(1), dim3(256), 0, s, cosv, sum, rows);
  return mmvae_launch_status();
}

// ---- sentence features -------------------------------------------------------------------------------------------------------
#define SF_EPL (MMVAE_SENTENCE_MAX_E / 64)      // elements of a feature per lane

// grid ceil(B / 4), 256 threads: wave = sentence, lane l holds the elements l, l + 64, ...
__global__ __launch_bounds__(256) void sentence_kernel(const int* __restrict__ ids, const float* __restrict__ emb,
                                                       const float* __restrict__ weights, const double* __restrict__ pc,
                                                       float* __restrict__ out, long B, int T, int E, int V, int eos) {
  const int lane = threadIdx.x & 63;
  const long sidx = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sidx >= B) return;      // (wave-uniform; no barrier)
  const int* __restrict__ row = ids + (size_t)sidx * T;
  int first = T;               // the first eos: per-lane strided scan, then the smallest over the wave
  for (int t = lane; t < T; t += 64)
    if (row[t] == eos) {
      first = t;
      break;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  const int L = first < T ? first + 1 : T;
  double f[SF_EPL];
#pragma unroll
  for (int e = 0; e < SF_EPL; ++e) f[e] = 0.0;
  for (int t = 0; t < L; ++t) {
    const int id = row[t];
    if ((unsigned)id >= (unsigned)V) continue;      // (the caller checks the ids; nothing is read outside the tables)
    const double w = (double)weights[id];
    const float* __restrict__ v = emb + (size_t)id * E;
#pragma unroll
    for (int e = 0; e < SF_EPL; ++e) {
      const int j = lane + 64 * e;
      if (j < E) f[e] += w * (double)v[j];
    }
  }
  double dot = 0.0;
#pragma unroll
  for (int e = 0; e < SF_EPL; ++e) {
    const int j = lane + 64 * e;
    f[e] /= (double)L;
    if (pc && j < E) dot += pc[j] * f[e];
  }
  if (pc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
  }
#pragma unroll
  for (int e = 0; e < SF_EPL; ++e) {
    const int j = lane + 64 * e;
    if (j < E) out[(size_t)sidx * E + j] = (float)(pc ? f[e] - pc[j] * dot : f[e]);
  }
}

extern "C" int mmvae_sentence_features(const int* ids, const float* emb, const float* weights, const double* pc, float* out,
                                       long B, int T, int E, int V, int eos, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(ids && emb && weights && out);
  if (B < 1 || B > MMVAE_CCA_MAX_ROWS || T < 1 || T > MMVAE_SENTENCE_MAX_T || E < 1 || E > MMVAE_SENTENCE_MAX_E || V < 1)
    return MMVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sentence_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ids, emb, weights, pc,
                     out, B, T, E, V, eos);
  return mmvae_launch_status();
}
