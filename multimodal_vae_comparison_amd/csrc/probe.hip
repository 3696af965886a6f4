// Latent classification (TorchMMVAE.classify_latents): linear probes on latent samples, trained and evaluated on chip.
//   mmvae_probe_train: ONE persistent workgroup per probe walks the minibatches of its steps itself -- logits, softmax,
//     mean cross-entropy, dW / db and the torch.optim.Adam update per step -- with W | b in LDS and the Adam moments in
//     registers; the next tile of latents is fetched into registers while the current one computes.
//   mmvae_probe_eval: row-parallel argmax + per-row cross-entropy of the trained probes.
// A probe's parameters are one (C, D + 1) matrix [W | b]: the bias is the weight of a constant-1 column that the latent
// tile carries in LDS, so the bias gradient and its Adam update are ordinary elements of the same loops.
#include "common.hpp"

#define PROBE_THREADS 256
#define PROBE_LDS_FLOATS 16384      // 64 KB: parameters of 32 classes + one latent tile + its logits + labels
#define PROBE_PF 32                 // prefetch registers per thread: a tile holds at most 256 * 32 latent elements
#define PROBE_EP 33                 // parameter elements per thread: 32 * 257 / 256 rounded up
#define PROBE_MISC 8

struct ProbeTable {
  int s[MMVAE_PROBE_MAX_PROBES], a[MMVAE_PROBE_MAX_PROBES], C[MMVAE_PROBE_MAX_PROBES];
};

__host__ __device__ __forceinline__ int probe_zs(int D) { return (D + 1) | 1; }      // odd row stride: no bank conflicts

// rows of a latent tile: a function of D alone (never of the launch), so that a probe computes the same sums whatever
// runs beside it.  Largest power of two <= 256 that fits the LDS budget and the prefetch registers; >= 16 for D <= 256.
__host__ __device__ __forceinline__ int probe_tile_rows(int D) {
  int tr = 256;
  while (tr > 16 && (tr * D > PROBE_THREADS * PROBE_PF ||
                     MMVAE_PROBE_MAX_CLASSES * (D + 1) + tr * (probe_zs(D) + MMVAE_PROBE_MAX_CLASSES + 1) + PROBE_MISC >
                         PROBE_LDS_FLOATS))
    tr >>= 1;
  return tr;
}

// beta^t, t >= 1, by repeated squaring in double (a function of t alone: a resumed training repeats it bit for bit)
__device__ __forceinline__ double probe_powi(double b, long t) {
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// one tile of one step: rows [pos0, pos0 + rows) of epoch `epoch`
struct ProbeTile {
  long t;          // global step
  int k;           // tile of the step
  int pos0, rows;  // first position, rows of this tile
  int step_rows;   // rows of the whole minibatch
  int last;        // last tile of its step
  long epoch;
};

__device__ __forceinline__ ProbeTile probe_tile(long t, int k, int N, int batch, int spe, int TR) {
  ProbeTile x;
  x.t = t;
  x.k = k;
  x.epoch = t / spe;
  const int i = (int)(t - x.epoch * spe);
  const int b0 = i * batch;
  x.step_rows = min(batch, N - b0);
  x.pos0 = b0 + k * TR;
  x.rows = min(TR, x.step_rows - k * TR);
  x.last = (k + 1) * TR >= x.step_rows;
  return x;
}

// The whole training of one probe.  EP = parameter elements per thread (compile time: the moments and the gradient are
// register arrays); the kernel picks the smallest of three sizes that holds the probe's C (D + 1) elements.  The
// arithmetic and its order do not depend on EP.
template <int EP>
__device__ __forceinline__ void probe_train_body(float* lds, const ProbeTable& tab, float* __restrict__ state,
                                                 const float* __restrict__ z, const int* __restrict__ labels,
                                                 const int* __restrict__ order, float* __restrict__ loss, int N, int D,
                                                 int Cmax, int batch, long step0, int n_steps, float lr) {
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = tab.C[p];
  const float* __restrict__ zp = z + (size_t)tab.s[p] * N * D;
  const int* __restrict__ lp = labels + (size_t)tab.a[p] * N;
  const int D1 = D + 1, ZS = probe_zs(D), TR = probe_tile_rows(D), NE = C * D1;
  float* Wl = lds;                                        // (C, D1): [W | b]
  float* zt = Wl + MMVAE_PROBE_MAX_CLASSES * D1;          // (TR, ZS): latent tile, column D = 1
  float* lg = zt + TR * ZS;                               // (C, TR): logits, then dlogit
  int* lab = (int*)(lg + TR * MMVAE_PROBE_MAX_CLASSES);   // (TR)
  float* misc = (float*)(lab + TR);                       // [0..3] loss partials of the waves, [4] lr / bc1, [5] sqrt(bc2)
  const size_t sstride = (size_t)Cmax * D1;
  float* st = state + (size_t)p * 3 * sstride;
  const int spe = (N + batch - 1) / batch;
  const long t_end = step0 + n_steps;

  // parameters -> LDS, moments -> registers; element e = tid + 256 j is (class e / D1, column e % D1)
  float m[EP], v[EP], g[EP];
  int eo[EP];      // (class * TR) << 16 | column: where the element's dlogit row and latent column start in LDS
  {
    int c = tid / D1, d = tid - c * D1;
    const int cq = PROBE_THREADS / D1, dq = PROBE_THREADS - cq * D1;
#pragma unroll
    for (int j = 0; j < EP; ++j) {
      const int e = tid + PROBE_THREADS * j;
      const bool in = e < NE;
      m[j] = in ? st[sstride + e] : 0.f;
      v[j] = in ? st[2 * sstride + e] : 0.f;
      g[j] = 0.f;
      if (in) Wl[e] = st[e];
      eo[j] = in ? (((c * TR) << 16) | d) : 0;
      d += dq;
      c += cq;
      if (d >= D1) {
        d -= D1;
        c += 1;
      }
    }
  }
  for (int r = tid; r < TR; r += PROBE_THREADS) zt[r * ZS + D] = 1.0f;

  // the thread's first tile element q = tid is (row r0, column d0); q += 256 moves it by (rq rows, dq columns)
  const int r0 = tid / D, d0 = tid - r0 * D;
  const int rq = PROBE_THREADS / D, dq = PROBE_THREADS - rq * D;
  float pf[PROBE_PF];
  int plab = 0;

  auto prefetch = [&](const ProbeTile& x) {
    const int n_el = x.rows * D;
    const int* __restrict__ ord = order ? order + (size_t)x.epoch * N + x.pos0 : nullptr;
    int r = r0, d = d0;
#pragma unroll
    for (int i = 0; i < PROBE_PF; ++i) {
      if (i * PROBE_THREADS < n_el) {      // (wave-uniform)
        const int q = tid + PROBE_THREADS * i;
        if (q < n_el) {
          const size_t row = ord ? (size_t)ord[r] : (size_t)(x.pos0 + r);
          pf[i] = zp[row * D + d];
        }
        d += dq;
        r += rq;
        if (d >= D) {
          d -= D;
          r += 1;
        }
      }
    }
    if (tid < x.rows) plab = lp[ord ? ord[tid] : x.pos0 + tid];
  };
  auto store = [&](const ProbeTile& x) {
    const int n_el = x.rows * D;
    int r = r0, d = d0;
#pragma unroll
    for (int i = 0; i < PROBE_PF; ++i) {
      if (i * PROBE_THREADS < n_el) {
        const int q = tid + PROBE_THREADS * i;
        if (q < n_el) zt[r * ZS + d] = pf[i];
        d += dq;
        r += rq;
        if (d >= D) {
          d -= D;
          r += 1;
        }
      }
    }
    if (tid < x.rows) lab[tid] = plab;
  };

  const float b1 = 0.9f, b2 = 0.999f, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
  ProbeTile cur = probe_tile(step0, 0, N, batch, spe, TR);
  prefetch(cur);
  float loss_acc = 0.f;
  while (cur.t < t_end) {
    store(cur);
    ProbeTile nxt = cur.last ? probe_tile(cur.t + 1, 0, N, batch, spe, TR) : probe_tile(cur.t, cur.k + 1, N, batch, spe, TR);
    if (nxt.t < t_end) prefetch(nxt);
    __syncthreads();      // 1: the tile (and, the first time, the parameters) are in LDS

    // logits: one (class, block of 64 rows) per wave and pass, over the rows the tile HAS; the lanes of a wave share the
    // class (W broadcast) and walk the rows (odd stride); logit of (class, row) at class * TR + row
    {
      const int nb = (cur.rows + 63) >> 6;
      for (int ws = wave; ws < C * nb; ws += PROBE_THREADS / 64) {
        const int c = ws / nb, r = ((ws - c * nb) << 6) + lane;
        if (r < cur.rows) {
          const float* __restrict__ zr = zt + r * ZS;
          const float* __restrict__ wc = Wl + c * D1;
          float acc = 0.f;
#pragma unroll 8
          for (int d = 0; d < D1; ++d) acc = fmaf(zr[d], wc[d], acc);
          lg[c * TR + r] = acc;
        }
      }
    }
    __syncthreads();      // 2: logits

    // softmax + cross-entropy of row tid; dlogit = (p - onehot) / rows of the minibatch, in place
    float lrow = 0.f;
    if (tid < cur.rows) {
      float mx = -INFINITY;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, lg[c * TR + tid]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += expf(lg[c * TR + tid] - mx);
      const float lse = mx + logf(s), inv_s = 1.0f / s, inv_rows = 1.0f / (float)cur.step_rows;
      const int y = lab[tid];
      for (int c = 0; c < C; ++c) {
        const float x = lg[c * TR + tid];
        if (c == y) lrow = lse - x;
        lg[c * TR + tid] = (expf(x - mx) * inv_s - (c == y ? 1.0f : 0.0f)) * inv_rows;
      }
    }
    lrow = wave_sum(lrow);
    if (lane == 0) misc[wave] = lrow;
    if (cur.last && tid == PROBE_THREADS - 1) {      // Adam's bias corrections of step t + 1
      const double bc1 = 1.0 - probe_powi(0.9, cur.t + 1), bc2 = 1.0 - probe_powi(0.999, cur.t + 1);
      misc[4] = (float)((double)lr / bc1);
      misc[5] = (float)sqrt(bc2);
    }
    __syncthreads();      // 3: dlogit, loss partials, bias corrections

    // dW | db: every thread sums its own elements over the rows, in row order
    for (int r = 0; r < cur.rows; ++r) {
      const float* __restrict__ zr = zt + r * ZS;
      const float* __restrict__ dl = lg + r;
#pragma unroll
      for (int j = 0; j < EP; ++j)
        if (j * PROBE_THREADS < NE) g[j] = fmaf(dl[eo[j] >> 16], zr[eo[j] & 0xFFFF], g[j]);      // (wave-uniform)
    }
    if (tid == 0) loss_acc += (misc[0] + misc[1]) + (misc[2] + misc[3]);
    if (cur.last) {
      const float step_size = misc[4], sq_bc2 = misc[5];
#pragma unroll
      for (int j = 0; j < EP; ++j) {
        const int e = tid + PROBE_THREADS * j;
        if (e < NE) {
          const float gg = g[j];
          m[j] = b1 * m[j] + omb1 * gg;
          v[j] = b2 * v[j] + omb2 * (gg * gg);
          const float denom = sqrtf(v[j]) / sq_bc2 + eps;
          Wl[e] -= step_size * (m[j] / denom);
        }
        g[j] = 0.f;
      }
      if (tid == 0) {
        loss[(size_t)p * n_steps + (cur.t - step0)] = loss_acc / (float)cur.step_rows;
        loss_acc = 0.f;
      }
    }
    __syncthreads();      // 4: the tile is free, the updated parameters are visible
    cur = nxt;
  }
#pragma unroll
  for (int j = 0; j < EP; ++j) {
    const int e = tid + PROBE_THREADS * j;
    if (e < NE) {
      st[e] = Wl[e];
      st[sstride + e] = m[j];
      st[2 * sstride + e] = v[j];
    }
  }
}

__global__ __launch_bounds__(PROBE_THREADS) void probe_train_kernel(ProbeTable tab, float* __restrict__ state,
                                                                    const float* __restrict__ z,
                                                                    const int* __restrict__ labels,
                                                                    const int* __restrict__ order,
                                                                    float* __restrict__ loss, int N, int D, int Cmax,
                                                                    int batch, long step0, int n_steps, float lr) {
  __shared__ float lds[PROBE_LDS_FLOATS];
  const int NE = tab.C[blockIdx.x] * (D + 1);
  if (NE <= PROBE_THREADS)
    probe_train_body<1>(lds, tab, state, z, labels, order, loss, N, D, Cmax, batch, step0, n_steps, lr);
  else if (NE <= 4 * PROBE_THREADS)
    probe_train_body<4>(lds, tab, state, z, labels, order, loss, N, D, Cmax, batch, step0, n_steps, lr);
  else
    probe_train_body<PROBE_EP>(lds, tab, state, z, labels, order, loss, N, D, Cmax, batch, step0, n_steps, lr);
}

// grid (row tiles, probes): the tile in LDS, one thread per row, all C logits of the row in registers
__global__ __launch_bounds__(PROBE_THREADS) void probe_eval_kernel(ProbeTable tab, const float* __restrict__ state,
                                                                   const float* __restrict__ z,
                                                                   const int* __restrict__ labels, int* __restrict__ pred,
                                                                   float* __restrict__ nll, int N, int D, int Cmax) {
  extern __shared__ float lds[];      // [W | b] of 32 classes + one latent tile: probe_eval_lds_floats(D)
  const int p = blockIdx.y, tid = threadIdx.x;
  const int C = tab.C[p];
  const int D1 = D + 1, ZS = probe_zs(D), TR = probe_tile_rows(D), NE = C * D1;
  const int pos0 = blockIdx.x * TR, rows = min(TR, N - pos0);
  float* Wl = lds;
  float* zt = Wl + MMVAE_PROBE_MAX_CLASSES * D1;
  const float* __restrict__ st = state + (size_t)p * 3 * Cmax * D1;
  const float* __restrict__ zp = z + ((size_t)tab.s[p] * N + pos0) * D;
  for (int e = tid; e < NE; e += PROBE_THREADS) Wl[e] = st[e];
  for (int r = tid; r < rows; r += PROBE_THREADS) zt[r * ZS + D] = 1.0f;
  {
    const int n_el = rows * D;
    int r = tid / D, d = tid - r * D;
    const int rq = PROBE_THREADS / D, dq = PROBE_THREADS - rq * D;
    for (int q = tid; q < n_el; q += PROBE_THREADS) {
      zt[r * ZS + d] = zp[q];
      d += dq;
      r += rq;
      if (d >= D) {
        d -= D;
        r += 1;
      }
    }
  }
  __syncthreads();
  if (tid >= rows) return;
  float acc[MMVAE_PROBE_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < MMVAE_PROBE_MAX_CLASSES; ++c) acc[c] = 0.f;
  const float* __restrict__ zr = zt + tid * ZS;
  for (int d = 0; d < D1; ++d) {
    const float zv = zr[d];
#pragma unroll
    for (int c = 0; c < MMVAE_PROBE_MAX_CLASSES; ++c)
      if (c < C) acc[c] = fmaf(zv, Wl[c * D1 + d], acc[c]);
  }
  float mx = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < MMVAE_PROBE_MAX_CLASSES; ++c)
    if (c < C && acc[c] > mx) {      // strict: the first maximum wins
      mx = acc[c];
      arg = c;
    }
  const size_t o = (size_t)p * N + pos0 + tid;
  pred[o] = arg;
  float out = 0.f;
  if (labels) {
    const int y = labels[(size_t)tab.a[p] * N + pos0 + tid];
    float s = 0.f, xy = 0.f;
#pragma unroll
    for (int c = 0; c < MMVAE_PROBE_MAX_CLASSES; ++c)
      if (c < C) {
        s += expf(acc[c] - mx);
        if (c == y) xy = acc[c];
      }
    out = mx + logf(s) - xy;
  }
  nll[o] = out;
}

static size_t probe_eval_lds_floats(int D) {
  return (size_t)MMVAE_PROBE_MAX_CLASSES * (D + 1) + (size_t)probe_tile_rows(D) * probe_zs(D);
}

extern "C" int mmvae_probe_tile_rows(int D) { return D >= 1 && D <= 256 ? probe_tile_rows(D) : 0; }

// the probe table (HOST, (P,3) = s, a, C per probe) by value into the launch; MMVAE_OK or the refusal
static int probe_table(const int* probes, int P, int S, int A, bool need_labels, int D, int Cmax, ProbeTable* t) {
  if (P > MMVAE_PROBE_MAX_PROBES || D > 256 || Cmax < 2 || Cmax > MMVAE_PROBE_MAX_CLASSES) return MMVAE_ERR_UNSUPPORTED;
  for (int i = 0; i < P; ++i) {
    const int s = probes[3 * i], a = probes[3 * i + 1], C = probes[3 * i + 2];
    if (C < 2 || C > Cmax || s < 0 || s >= S || a < 0 || (need_labels && a >= A)) return MMVAE_ERR_UNSUPPORTED;
    t->s[i] = s;
    t->a[i] = a;
    t->C[i] = C;
  }
  return MMVAE_OK;
}

extern "C" int mmvae_probe_train(float* state, const float* z, const int* labels, const int* order, int order_epochs,
                                 const int* probes, float* loss, int P, int S, int A, int N, int D, int Cmax, int batch,
                                 long step0, int n_steps, float lr, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && z && labels && probes && loss && P > 0 && S > 0 && A > 0 && N > 0 && D > 0 && step0 >= 0 &&
                  n_steps > 0);
  if (batch < 1) return MMVAE_ERR_UNSUPPORTED;
  ProbeTable t;
  const int rc = probe_table(probes, P, S, A, true, D, Cmax, &t);
  if (rc != MMVAE_OK) return rc;
  const long spe = ((long)N + batch - 1) / batch;
  if (order) MMVAE_CHECK_ARG((step0 + n_steps - 1) / spe < order_epochs);
  hipLaunchKernelGGL(probe_train_kernel, dim3(P), dim3(PROBE_THREADS), 0, (hipStream_t)stream, t, state, z, labels, order,
                     loss, N, D, Cmax, batch, step0, n_steps, lr);
  return mmvae_launch_status();
}

extern "C" int mmvae_probe_eval(const float* state, const float* z, const int* labels, const int* probes, int* pred,
                                float* nll, int P, int S, int A, int N, int D, int Cmax, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && z && probes && pred && nll && P > 0 && S > 0 && N > 0 && D > 0 && (!labels || A > 0));
  ProbeTable t;
  const int rc = probe_table(probes, P, S, A, labels != nullptr, D, Cmax, &t);
  if (rc != MMVAE_OK) return rc;
  const int TR = probe_tile_rows(D);
  hipLaunchKernelGGL(probe_eval_kernel, dim3((N + TR - 1) / TR, P), dim3(PROBE_THREADS),
                     probe_eval_lds_floats(D) * sizeof(float), (hipStream_t)stream, t, state, z, labels, pred, nll, N, D, Cmax);
  return mmvae_launch_status();
}
