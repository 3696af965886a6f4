// Cross-modal retrieval of latents (TorchMMVAE.cross_modal_retrieval; ops.retrieval_ranks): per ordered pair (query set,
// gallery set) of S sets of N rows and per query row i, the distance d_match to its partner row match(i) of the gallery, how
// many other gallery rows are nearer (less) or exactly as near (equal), and its `keep` nearest gallery rows ordered by
// (distance, index) -- what recall@k, median rank and MRR read.  Distances in double from fp32 values converted on load, by
// direct differences (no Gram route: the widths are small and the distribution distances divide), dimensions in order:
//   l2      sum (mq - mg)^2                        cosine  1 - sum mq mg / sqrt(sum mq^2 . sum mg^2), 1 when a norm is 0
//   w2      sum (mq - mg)^2 + (sq - sg)^2          skl     sum 1/2 [(sq^2 + D^2) / sg^2 + (sg^2 + D^2) / sq^2] - 1, D = mq - mg
// ONE arithmetic per pair: RtAcc<M> (explicit fma, contraction off in this file) is stepped over the dimensions in order and
// read once, for the matched pair and for every other pair alike; its value is a function of the two rows and of nothing
// else (not of tile, chunk or launch shape), so that d_ij < d_match compares two values of one arithmetic.
//   rt_rank_kernel    grid (chunks, row tiles, pairs), 256 threads.  A workgroup owns 64 query rows (one per lane) and a chunk
//                     of gallery rows staged RT_MT = 32 at a time, the dimensions KD at a time, in LDS as doubles: the mean
//                     and, per metric, the scale or the variance and its reciprocal (one divide per staged element, none per
//                     pair); the query rows lie beside them in the same form (staged once when D <= KD).  Wave q owns 8 of the
//                     32 staged rows: a thread steps 8 accumulators per dimension (every gallery read a broadcast), then
//                     compares the 8 distances with its row's d_match and offers them to its sorted list.  d_match first: wave 0
//                     walks each row's partner straight from memory with the same accumulator.  The four waves' counts and
//                     lists are merged in wave order through LDS.
//   rt_merge_kernel   the chunks' partials merged in chunk order, one thread per (pair, row); not launched for one chunk
// The N x N distances are never written.  No atomics.  What is merged are integer sums and "the keep smallest by (d, index)":
// the outputs are the same bits under any column split, and for a pair alone or beside other pairs in the launch.
#include <math.h>

#include "common.hpp"

#pragma clang fp contract(off)

#define RT_ROWS 64                 // query rows of a workgroup: one per lane
#define RT_MT 32                   // gallery rows of a staged tile
#define RT_WR (RT_MT / 4)          // gallery rows of a wave
#define RT_GLD (RT_MT + 2)         // LDS stride of a staged dimension of the gallery tile, in doubles (16-byte groups of 8 rows)
#define RT_SLOTS 1024              // workgroups wanted: 256 CUs x 4
#define RT_MIN_TILES 8             // staged tiles per chunk at least (a workgroup's walk of its partners costs about one)
#define RT_KEEP MMVAE_RETRIEVAL_MAX_KEEP

static bool rt_ok(long N, int P, int keep, int chunks) {
  return N >= 1 && N <= MMVAE_RETRIEVAL_MAX_ROWS && P >= 1 && P <= MMVAE_RETRIEVAL_MAX_PAIRS && keep >= 0 &&
         keep <= MMVAE_RETRIEVAL_MAX_KEEP && chunks >= 0;
}
static int rt_row_tiles(long N) { return (int)((N + RT_ROWS - 1) / RT_ROWS); }

// -> staged tiles per chunk and the chunks that hold at least one tile; `chunks` 0: the default plan
static void rt_plan(long N, int P, int chunks, int* tiles_per_chunk, int* n_chunks) {
  const int ct = (int)((N + RT_MT - 1) / RT_MT);
  if (chunks <= 0) {
    const long wg = (long)rt_row_tiles(N) * P;
    chunks = (int)((RT_SLOTS + wg - 1) / wg);
    const int most = (ct + RT_MIN_TILES - 1) / RT_MIN_TILES;
    if (chunks > most) chunks = most;
  }
  if (chunks > ct) chunks = ct;
  *tiles_per_chunk = (ct + chunks - 1) / chunks;
  *n_chunks = (ct + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

// ---- the one arithmetic of a pair -------------------------------------------------------------------------------------------
template <int M>
struct RtForm {
  static constexpr int NCH = M == MMVAE_RETRIEVAL_SKL ? 3 : (M == MMVAE_RETRIEVAL_W2 ? 2 : 1);      // doubles per element
  static constexpr int KD = M == MMVAE_RETRIEVAL_SKL ? 16 : 32;      // dimensions of a staged step (64 KB of LDS at most)
  static constexpr bool SCALED = NCH > 1;
};

// what an element gives every pair it is in: the mean; w2: the scale; skl: the variance and its reciprocal
template <int M>
__device__ __forceinline__ void rt_element(float mu, float sigma, double* c) {
  c[0] = (double)mu;
  if constexpr (M == MMVAE_RETRIEVAL_W2) c[1] = (double)sigma;
  if constexpr (M == MMVAE_RETRIEVAL_SKL) {
    const double s = (double)sigma;
    c[1] = s * s;
    c[2] = 1.0 / c[1];
  }
}

// stepped over the dimensions in order with the elements of the query row (q) and of the gallery row (g), then read
template <int M>
struct RtAcc {
  double a, ng;      // ng: the gallery row's squared norm (cosine)
  __device__ __forceinline__ void clear() { a = 0.0, ng = 0.0; }
  __device__ __forceinline__ void step(const double* q, const double* g) {
    if constexpr (M == MMVAE_RETRIEVAL_COSINE) {
      a = fma(q[0], g[0], a);
      ng = fma(g[0], g[0], ng);
    } else {
      const double d = q[0] - g[0];
      if constexpr (M == MMVAE_RETRIEVAL_L2) a = fma(d, d, a);
      if constexpr (M == MMVAE_RETRIEVAL_W2) {
        const double e = q[1] - g[1];
        a = fma(d, d, a);
        a = fma(e, e, a);
      }
      if constexpr (M == MMVAE_RETRIEVAL_SKL) {
        double t = fma(d, d, q[1]) * g[2];
        t = fma(fma(d, d, g[1]), q[2], t);
        a = fma(0.5, t, a);
      }
    }
  }
  // nq: the query row's squared norm, sum of fma(q, q, .) in dimension order (cosine)
  __device__ __forceinline__ double value(double nq, int D) const {
    if constexpr (M == MMVAE_RETRIEVAL_COSINE) return (nq == 0.0 || ng == 0.0) ? 1.0 : 1.0 - a / sqrt(nq * ng);
    if constexpr (M == MMVAE_RETRIEVAL_SKL) return a - (double)D;
    return a;
  }
};

// ---- a list of the KEEP nearest, sorted by (distance, index), in registers --------------------------------------------------------
// (every index is a compile-time constant after unrolling; empty slots hold (+inf, -1), which sorts behind every row)
__device__ __forceinline__ bool rt_before(double x, int j, double d, int i) {
  return x < d || (x == d && (unsigned)j < (unsigned)i);
}
template <int KEEP>
struct RtKeep {
  double d[KEEP > 0 ? KEEP : 1];
  int i[KEEP > 0 ? KEEP : 1];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < KEEP; ++s) d[s] = INFINITY, i[s] = -1;
  }
  __device__ __forceinline__ void put(double x, int j) {
    if constexpr (KEEP > 0) {
      if (!rt_before(x, j, d[KEEP - 1], i[KEEP - 1])) return;
#pragma unroll
      for (int s = 0; s < KEEP; ++s) {
        const bool first = rt_before(x, j, d[s], i[s]);
        const double od = d[s];
        const int oi = i[s];
        d[s] = first ? x : od;
        i[s] = first ? j : oi;
        x = first ? od : x;
        j = first ? oi : j;
      }
    }
  }
};

// the partner of query row i: match[i], or i without a list; -1 (no partner) for anything outside [0, N)
__device__ __forceinline__ int rt_partner(const int* __restrict__ match, long i, long N) {
  const int m = match ? match[i] : (int)i;
  return (m < 0 || m >= N) ? -1 : m;
}

// ---- ranks and neighbours of a chunk ------------------------------------------------------------------------------------------
// less, equal (chunk, P, N) and nn_d, nn_idx (chunk, P, N, keep): the outputs themselves when there is one chunk (`final`:
// rows without a partner get -1), the workspace otherwise; d_match (P, N) is written by chunk 0
template <int M, int KEEP>
__global__ __launch_bounds__(256) void rt_rank_kernel(const float* __restrict__ loc, const float* __restrict__ scale,
                                                      const int* __restrict__ pairs, const int* __restrict__ match,
                                                      double* __restrict__ d_match, int* __restrict__ less_out,
                                                      int* __restrict__ equal_out, double* __restrict__ nn_d,
                                                      int* __restrict__ nn_idx, long N, int D, int S, int keep, int tpc,
                                                      int final) {
  constexpr int NCH = RtForm<M>::NCH, KD = RtForm<M>::KD, QLD = KD + 1;
  constexpr bool SCALED = RtForm<M>::SCALED;
  constexpr int G_DOUBLES = NCH * KD * RT_GLD, Q_DOUBLES = NCH * RT_ROWS * QLD;
  constexpr int MERGE_DOUBLES = RT_KEEP * RT_ROWS + (RT_KEEP * RT_ROWS + 2 * RT_ROWS) / 2;
  static_assert(MERGE_DOUBLES <= G_DOUBLES + Q_DOUBLES, "the waves' lists fit inside the staged tiles");
  static_assert((G_DOUBLES + Q_DOUBLES + RT_ROWS) * 8 <= 64 * 1024, "static LDS");
  __shared__ double lds[G_DOUBLES + Q_DOUBLES];
  __shared__ double dm_s[RT_ROWS];
  double* g_s = lds;                      // [ch][dd][RT_GLD]
  double* q_s = lds + G_DOUBLES;          // [ch][row][QLD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.z;
  const int qset = pairs[2 * p], gset = pairs[2 * p + 1];
  if ((unsigned)qset >= (unsigned)S || (unsigned)gset >= (unsigned)S) return;      // (the whole workgroup)
  const size_t set = (size_t)N * D;
  const float *qloc = loc + qset * set, *gloc = loc + gset * set;
  const float *qsc = SCALED ? scale + qset * set : nullptr, *gsc = SCALED ? scale + gset * set : nullptr;
  const long i0 = (long)blockIdx.y * RT_ROWS, row = i0 + lane;
  const bool live = row < N;
  const int mine = live ? rt_partner(match, row, N) : -1;

  // d_match: the partner's row straight from memory, the same accumulator
  if (wave == 0) {
    double dm = NAN;
    if (mine >= 0) {
      RtAcc<M> acc;
      acc.clear();
      double nq = 0.0;
      const size_t qa = (size_t)row * D, ga = (size_t)mine * D;
      for (int d = 0; d < D; ++d) {
        double q[NCH], g[NCH];
        rt_element<M>(qloc[qa + d], SCALED ? qsc[qa + d] : 1.0f, q);
        rt_element<M>(gloc[ga + d], SCALED ? gsc[ga + d] : 1.0f, g);
        if constexpr (M == MMVAE_RETRIEVAL_COSINE) nq = fma(q[0], q[0], nq);
        acc.step(q, g);
      }
      dm = acc.value(nq, D);
    }
    dm_s[lane] = dm;
    if (blockIdx.x == 0 && live) d_match[(size_t)p * N + row] = dm;
  }
  __syncthreads();
  const double dm = dm_s[lane];

  int less = 0, equal = 0;
  RtKeep<KEEP> near;
  near.clear();
  const bool q_once = D <= KD;
  const int ct = (int)((N + RT_MT - 1) / RT_MT);
  const int t0 = blockIdx.x * tpc, t1 = min(ct, t0 + tpc);
  for (int t = t0; t < t1; ++t) {
    const long m0 = (long)t * RT_MT;
    RtAcc<M> acc[RT_WR];
#pragma unroll
    for (int i = 0; i < RT_WR; ++i) acc[i].clear();
    double nq = 0.0;
    for (int db = 0; db < D; db += KD) {
      __syncthreads();      // (the previous step has been read)
#pragma unroll
      for (int e = 0; e < RT_MT * KD / 256; ++e) {
        const int idx = tid + 256 * e, r = idx / KD, dd = idx % KD;
        double c[NCH];
        if (m0 + r < N && db + dd < D) {
          const size_t at = (size_t)(m0 + r) * D + db + dd;
          rt_element<M>(gloc[at], SCALED ? gsc[at] : 1.0f, c);
        } else {
          rt_element<M>(0.0f, 1.0f, c);
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) g_s[(ch * KD + dd) * RT_GLD + r] = c[ch];
      }
      if (!q_once || t == t0) {
#pragma unroll
        for (int e = 0; e < RT_ROWS * KD / 256; ++e) {
          const int idx = tid + 256 * e, r = idx / KD, dd = idx % KD;
          double c[NCH];
          if (i0 + r < N && db + dd < D) {
            const size_t at = (size_t)(i0 + r) * D + db + dd;
            rt_element<M>(qloc[at], SCALED ? qsc[at] : 1.0f, c);
          } else {
            rt_element<M>(0.0f, 1.0f, c);
          }
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) q_s[(ch * RT_ROWS + r) * QLD + dd] = c[ch];
        }
      }
      __syncthreads();
      const int dims = min(KD, D - db);
      for (int dd = 0; dd < dims; ++dd) {
        double q[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) q[ch] = q_s[(ch * RT_ROWS + lane) * QLD + dd];
        if constexpr (M == MMVAE_RETRIEVAL_COSINE) nq = fma(q[0], q[0], nq);
#pragma unroll
        for (int i = 0; i < RT_WR; ++i) {
          double g[NCH];
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) g[ch] = g_s[(ch * KD + dd) * RT_GLD + wave * RT_WR + i];
          acc[i].step(q, g);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < RT_WR; ++i) {
      const long j = m0 + wave * RT_WR + i;
      if (j < N) {
        const double d = acc[i].value(nq, D);
        if (j != mine) {
          less += d < dm ? 1 : 0;
          equal += d == dm ? 1 : 0;
        }
        near.put(d, (int)j);
      }
    }
  }

  // the four waves' counts and lists, in wave order (the lists take the staged tiles' place)
  double* m_d = lds;                                                            // [slot][lane]
  int* m_i = reinterpret_cast<int*>(lds + RT_KEEP * RT_ROWS);                   // [slot][lane], then less, equal [lane]
  int* m_c = m_i + RT_KEEP * RT_ROWS;
  for (int w = 1; w < 4; ++w) {
    __syncthreads();        // (the last step, or wave 0's merge of the previous wave, has read the LDS)
    if (wave == w) {
      m_c[lane] = less;
      m_c[RT_ROWS + lane] = equal;
#pragma unroll
      for (int s = 0; s < KEEP; ++s) {
        m_d[s * RT_ROWS + lane] = near.d[s];
        m_i[s * RT_ROWS + lane] = near.i[s];
      }
    }
    __syncthreads();
    if (wave == 0) {
      less += m_c[lane];
      equal += m_c[RT_ROWS + lane];
#pragma unroll
      for (int s = 0; s < KEEP; ++s) near.put(m_d[s * RT_ROWS + lane], m_i[s * RT_ROWS + lane]);
    }
  }
  if (wave != 0 || !live) return;
  const size_t at = ((size_t)blockIdx.x * gridDim.z + p) * N + row;
  const bool none = final && mine < 0;
  less_out[at] = none ? -1 : less;
  equal_out[at] = none ? -1 : equal;
#pragma unroll
  for (int s = 0; s < KEEP; ++s)
    if (s < keep) {
      nn_d[at * keep + s] = near.d[s];
      nn_idx[at * keep + s] = near.i[s];
    }
}

// ---- the chunks in order: one thread per (pair, row) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rt_merge_kernel(const int* __restrict__ match, const int* __restrict__ part_less,
                                                       const int* __restrict__ part_equal, const double* __restrict__ part_d,
                                                       const int* __restrict__ part_i, int* __restrict__ less_out,
                                                       int* __restrict__ equal_out, double* __restrict__ nn_d,
                                                       int* __restrict__ nn_idx, long N, int P, int keep, int chunks) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)P * N) return;
  const long row = idx % N;
  int less = 0, equal = 0;
  RtKeep<RT_KEEP> near;
  near.clear();
  for (int c = 0; c < chunks; ++c) {
    const size_t at = (size_t)c * P * N + idx;
    less += part_less[at];
    equal += part_equal[at];
    for (int s = 0; s < keep; ++s) near.put(part_d[at * keep + s], part_i[at * keep + s]);
  }
  const bool none = rt_partner(match, row, N) < 0;
  less_out[idx] = none ? -1 : less;
  equal_out[idx] = none ? -1 : equal;
#pragma unroll
  for (int s = 0; s < RT_KEEP; ++s)
    if (s < keep) {
      nn_d[(size_t)idx * keep + s] = near.d[s];
      nn_idx[(size_t)idx * keep + s] = near.i[s];
    }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" int mmvae_retrieval_chunks(long N, int P) {
  if (!rt_ok(N, P, 0, 0)) return 0;
  int tpc, n;
  rt_plan(N, P, 0, &tpc, &n);
  return n;
}

extern "C" size_t mmvae_retrieval_ws_bytes(long N, int P, int keep, int chunks) {
  if (!rt_ok(N, P, keep, chunks)) return 0;
  int tpc, n;
  rt_plan(N, P, chunks, &tpc, &n);
  if (n == 1) return 0;
  const size_t rows = (size_t)n * P * N;
  return rows * keep * sizeof(double) + (rows * (2 + (size_t)keep) * sizeof(int) + 7) / 8 * 8;      // (whole doubles)
}

template <int M>
static void rt_launch(const float* loc, const float* scale, const int* pairs, const int* match, double* d_match, int* less,
                      int* equal, double* nn_d, int* nn_idx, long N, int D, int S, int P, int keep, int tpc, int n,
                      hipStream_t s) {
  const dim3 grid(n, rt_row_tiles(N), P);
  const int final = n == 1;
  if (keep > 0)
    hipLaunchKernelGGL((rt_rank_kernel<M, RT_KEEP>), grid, dim3(256), 0, s, loc, scale, pairs, match, d_match, less, equal,
                       nn_d, nn_idx, N, D, S, keep, tpc, final);
  else
    hipLaunchKernelGGL((rt_rank_kernel<M, 0>), grid, dim3(256), 0, s, loc, scale, pairs, match, d_match, less, equal, nn_d,
                       nn_idx, N, D, S, keep, tpc, final);
}

extern "C" int mmvae_retrieval_ranks(const float* loc, const float* scale, const int* pairs, const int* match, void* ws,
                                     double* d_match, int* less, int* equal, double* nn_d, int* nn_idx, long N, int D, int S,
                                     int P, int metric, int keep, int chunks, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(loc && pairs && d_match && less && equal);
  if (!rt_ok(N, P, keep, chunks) || D < 1 || D > MMVAE_RETRIEVAL_MAX_DIM || S < 2 || S > MMVAE_RETRIEVAL_MAX_SETS ||
      metric < MMVAE_RETRIEVAL_L2 || metric > MMVAE_RETRIEVAL_SKL)
    return MMVAE_ERR_UNSUPPORTED;
  MMVAE_CHECK_ARG(keep == 0 || (nn_d && nn_idx));
  MMVAE_CHECK_ARG(scale || (metric != MMVAE_RETRIEVAL_W2 && metric != MMVAE_RETRIEVAL_SKL));
  int tpc, n;
  rt_plan(N, P, chunks, &tpc, &n);
  MMVAE_CHECK_ARG(n == 1 || ws);
  hipStream_t s = (hipStream_t)stream;
  // one chunk: the kernel writes the outputs; more: (chunk, P, N, keep) doubles | the same ints | less | equal of the workspace
  const size_t rows = (size_t)n * P * N;
  double* part_d = n == 1 ? nn_d : static_cast<double*>(ws);
  int* part_i = n == 1 ? nn_idx : reinterpret_cast<int*>(static_cast<double*>(ws) + rows * keep);
  int* part_less = n == 1 ? less : reinterpret_cast<int*>(static_cast<double*>(ws) + rows * keep) + rows * keep;
  int* part_equal = n == 1 ? equal : part_less + rows;
  switch (metric) {
    case MMVAE_RETRIEVAL_L2:
      rt_launch<MMVAE_RETRIEVAL_L2>(loc, scale, pairs, match, d_match, part_less, part_equal, part_d, part_i, N, D, S, P, keep,
                                    tpc, n, s);
      break;
    case MMVAE_RETRIEVAL_COSINE:
      rt_launch<MMVAE_RETRIEVAL_COSINE>(loc, scale, pairs, match, d_match, part_less, part_equal, part_d, part_i, N, D, S, P,
                                        keep, tpc, n, s);
      break;
    case MMVAE_RETRIEVAL_W2:
      rt_launch<MMVAE_RETRIEVAL_W2>(loc, scale, pairs, match, d_match, part_less, part_equal, part_d, part_i, N, D, S, P, keep,
                                    tpc, n, s);
      break;
    default:
      rt_launch<MMVAE_RETRIEVAL_SKL>(loc, scale, pairs, match, d_match, part_less, part_equal, part_d, part_i, N, D, S, P, keep,
                                     tpc, n, s);
      break;
  }
  if (n > 1)
    hipLaunchKernelGGL(rt_merge_kernel, dim3((unsigned)(((long)P * N + 255) / 256)), dim3(256), 0, s, match, part_less,
                       part_equal, part_d, part_i, less, equal, nn_d, nn_idx, N, P, keep, n);
  return mmvae_launch_status();
}
