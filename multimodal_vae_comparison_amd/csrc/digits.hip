// MNIST-SVHN digit coherence (TorchMMVAE.digit_cross_coherence / digit_joint_coherence): the reference's two LeNet-style
// digit classifiers (eval/mnistsvhn_helper.py: MNIST_Classifier / SVHN_Classifier), evaluated and TRAINED on chip.
//   digit_image_kernel: ONE workgroup per image runs the whole network with every activation in LDS -- conv1 + max-pool +
//     ReLU, conv2 + Dropout2d + max-pool + ReLU, fc1 + ReLU + dropout, fc2, log-softmax -- and, when training, the whole
//     backward pass; it leaves the image's gradient of every parameter in its own row of a workspace.
//   digit_fold_kernel: sums those rows in a fixed order and applies torch.optim.Adam (or stores the reduced gradient).
// A training step is these two ordinary launches; no atomics, no barrier between workgroups.
// The pools are fused into the convolutions: a thread computes the four outputs of a window, keeps their first maximum
// (row-major, torch's rule) and remembers where it was, so that the pre-pool maps never exist.  Dropout2d's mask is >= 0,
// so it commutes with the max: relu(pool(m * y)) = relu(m * pool(y)), with the same first maximum whenever m > 0.
#include "common.hpp"

#define DG_THREADS 256
#define DG_LDS_FLOATS 15360      // 60 KB: the SVHN network's activations, gradients and conv weights (15 164 floats)

template <int CIN_, int H_>
struct DigitGeom {
  static constexpr int CIN = CIN_, H = H_;             // input (CIN, H, H)
  static constexpr int P1 = (H - 4) / 2;               // conv1 + pool: (10, P1, P1)
  static constexpr int P2 = (P1 - 4) / 2;              // conv2 + pool: (20, P2, P2)
  static constexpr int NX = CIN * H * H, NA1 = 10 * P1 * P1, FLAT = 20 * P2 * P2;
  static constexpr int NW1 = 10 * CIN * 25, NW2 = 20 * 10 * 25;
  // packed parameters: conv1.w, conv1.b, conv2.w, conv2.b, fc1.w, fc1.b, fc2.w, fc2.b
  static constexpr int W1 = 0, B1 = W1 + NW1, W2 = B1 + 10, B2 = W2 + NW2, F1W = B2 + 20, F1B = F1W + 50 * FLAT,
                       F2W = F1B + 50, F2B = F2W + 500, NPAR = F2B + 10;
  // LDS (floats)
  static constexpr int L_X = 0, L_W1 = L_X + NX, L_W2 = L_W1 + NW1, L_A1 = L_W2 + NW2, L_G1 = L_A1 + NA1,
                       L_A2 = L_G1 + NA1, L_G2 = L_A2 + FLAT, L_Q1 = L_G2 + FLAT, L_Q2 = L_Q1 + (NA1 + 1) / 2,
                       L_H = L_Q2 + (FLAT + 1) / 2, L_END = L_H + 192;
};
typedef DigitGeom<1, 28> DigitM;
typedef DigitGeom<3, 32> DigitS;
static_assert(DigitM::NPAR == 21840 && DigitS::NPAR == 31340, "parameter counts of the reference's classifiers");
static_assert(DigitS::L_END <= DG_LDS_FLOATS && DigitM::L_END <= DG_LDS_FLOATS, "LDS budget");

struct DigitTable {
  int kind[MMVAE_DIGIT_MAX_NETS];
  const float* x[MMVAE_DIGIT_MAX_NETS];
  const int* y[MMVAE_DIGIT_MAX_NETS];
};

static inline int digit_npar(int kind) { return kind == MMVAE_DIGIT_MNIST ? DigitM::NPAR : DigitS::NPAR; }

// The key of one dropout site of one network at one global step.  A mask element is drop_mul(key, row * units + unit):
// a function of (seed, network kind, step, position of the row in its minibatch, unit) and of nothing else.
__device__ __forceinline__ DropKey digit_key(uint32_t seed, int kind, long step, uint32_t site, float p) {
  DropKey k;
  k.on = p > 0.f;
  k.p = p;
  k.inv_keep = k.on ? 1.0f / (1.0f - p) : 1.0f;
  k.thr = (uint32_t)(p * 65536.0f + 0.5f);
  uint32_t h = drop_fmix(seed ^ ((uint32_t)kind * 0x85EBCA77u + site * 0xC2B2AE3Du + 0x27D4EB2Fu));
  h = drop_fmix(h + (uint32_t)((unsigned long)step & 0xFFFFFFFFul) * 0x9E3779B1u);
  h = drop_fmix(h ^ (uint32_t)((unsigned long)step >> 32));
  k.key = h;
  return k;
}

// first maximum of a 2x2 window in row-major order; q = its offset (dy << 1 | dx)
__device__ __forceinline__ float digit_max4(float a, float b, float c, float d, int& q) {
  float m = a;
  q = 0;
  if (b > m) { m = b; q = 1; }
  if (c > m) { m = c; q = 2; }
  if (d > m) { m = d; q = 3; }
  return m;
}

// The whole network on one image.  par: the packed parameters; x: the image; row: the image's position in its minibatch
// (dropout masks); gout (NPAR): the image's gradient of inv_rows * loss (TRAIN only).
template <class G, bool TRAIN, bool HIDDEN_ONLY = false>
__device__ __forceinline__ void digit_body(float* lds, const float* __restrict__ par, const float* __restrict__ x,
                                           int label, float inv_rows, const DropKey k2d, const DropKey k1, uint32_t row,
                                           float* __restrict__ gout, float* __restrict__ rowloss,
                                           float* __restrict__ logp_out, int* __restrict__ pred_out,
                                           float* __restrict__ hid_out = nullptr) {
  constexpr int H = G::H, CIN = G::CIN, P1 = G::P1, P2 = G::P2, PP1 = P1 * P1, PP2 = P2 * P2, FLAT = G::FLAT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* xs = lds + G::L_X;
  float* w1s = lds + G::L_W1;
  float* w2s = lds + G::L_W2;
  float* a1 = lds + G::L_A1;                            // relu(pool(conv1))
  float* g1 = lds + G::L_G1;                            // gradient of conv1's output at the window's maximum
  float* a2 = lds + G::L_A2;                            // relu(pool(dropout2d(conv2))), flattened (channel, y, x)
  float* g2 = lds + G::L_G2;                            // gradient of conv2's output at the window's maximum
  unsigned short* q1 = (unsigned short*)(lds + G::L_Q1);      // (y << 8 | x) of the maximum in conv1's output map
  unsigned short* q2 = (unsigned short*)(lds + G::L_Q2);      // ... in conv2's output map
  float* h1 = lds + G::L_H;                             // (50) dropout(relu(fc1))
  float* hm = h1 + 50;                                  // (50) its mask times the ReLU gate
  float* dh = hm + 50;                                  // (50) gradient of fc1's output
  float* lg = dh + 50;                                  // (10) logits, then log-probs
  float* dl = lg + 16;                                  // (10) gradient of the logits

  for (int i = tid; i < G::NX; i += DG_THREADS) xs[i] = x[i];
  for (int i = tid; i < G::NW1; i += DG_THREADS) w1s[i] = par[G::W1 + i];
  for (int i = tid; i < G::NW2; i += DG_THREADS) w2s[i] = par[G::W2 + i];
  __syncthreads();

  // conv1 (k5) + pool 2 + ReLU
  for (int o = tid; o < G::NA1; o += DG_THREADS) {
    const int oc = o / PP1, r = o - oc * PP1, py = r / P1, px = r - py * P1;
    const float b = par[G::B1 + oc];
    float c0 = b, c1 = b, c2 = b, c3 = b;
#pragma unroll 1
    for (int ic = 0; ic < CIN; ++ic) {
      const float* __restrict__ wp = w1s + (oc * CIN + ic) * 25;
      const float* __restrict__ xp = xs + ic * H * H + (2 * py) * H + 2 * px;
#pragma unroll
      for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
          const float w = wp[ky * 5 + kx];
          const float* __restrict__ s = xp + ky * H + kx;
          c0 = fmaf(w, s[0], c0);
          c1 = fmaf(w, s[1], c1);
          c2 = fmaf(w, s[H], c2);
          c3 = fmaf(w, s[H + 1], c3);
        }
    }
    int q;
    const float m = digit_max4(c0, c1, c2, c3, q);
    a1[o] = fmaxf(m, 0.f);
    q1[o] = (unsigned short)(((2 * py + (q >> 1)) << 8) | (2 * px + (q & 1)));
  }
  __syncthreads();

  // conv2 (k5) + Dropout2d + pool 2 + ReLU
  for (int o = tid; o < FLAT; o += DG_THREADS) {
    const int oc = o / PP2, r = o - oc * PP2, py = r / P2, px = r - py * P2;
    const float b = par[G::B2 + oc];
    float c0 = b, c1 = b, c2 = b, c3 = b;
#pragma unroll 1
    for (int ic = 0; ic < 10; ++ic) {
      const float* __restrict__ wp = w2s + (oc * 10 + ic) * 25;
      const float* __restrict__ ap = a1 + ic * PP1 + (2 * py) * P1 + 2 * px;
#pragma unroll
      for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
          const float w = wp[ky * 5 + kx];
          const float* __restrict__ s = ap + ky * P1 + kx;
          c0 = fmaf(w, s[0], c0);
          c1 = fmaf(w, s[1], c1);
          c2 = fmaf(w, s[P1], c2);
          c3 = fmaf(w, s[P1 + 1], c3);
        }
    }
    const float md = TRAIN ? drop_mul(k2d, row * 20u + (uint32_t)oc) : 1.0f;
    int q;
    const float m = digit_max4(c0, c1, c2, c3, q);
    a2[o] = fmaxf(md * m, 0.f);
    q2[o] = (unsigned short)(((2 * py + (q >> 1)) << 8) | (2 * px + (q & 1)));
  }
  __syncthreads();

  // fc1 + ReLU + dropout: one wave per output, the lanes walk the inputs
  for (int j = wave; j < 50; j += DG_THREADS / 64) {
    const float* __restrict__ wr = par + G::F1W + j * FLAT;
    float s = 0.f;
    for (int i = lane; i < FLAT; i += 64) s = fmaf(a2[i], wr[i], s);
    s = wave_sum(s);
    if (lane == 0) {
      const float h = s + par[G::F1B + j];
      const float md = TRAIN ? drop_mul(k1, row * 50u + (uint32_t)j) : 1.0f;
      h1[j] = fmaxf(h, 0.f) * md;
      hm[j] = h > 0.f ? md : 0.f;
      if (HIDDEN_ONLY) hid_out[j] = h1[j];
    }
  }
  if (HIDDEN_ONLY) return;      // (mmvae_digit_hidden: relu(fc1) is the output)
  __syncthreads();

  // fc2
  if (tid < 10) {
    const float* __restrict__ wr = par + G::F2W + tid * 50;
    float s = par[G::F2B + tid];
    for (int j = 0; j < 50; ++j) s = fmaf(h1[j], wr[j], s);
    lg[tid] = s;
  }
  __syncthreads();

  // log-softmax, prediction (the first maximum), loss and the logits' gradient
  if (tid == 0) {
    float mx = lg[0];
    int arg = 0;
    for (int c = 1; c < 10; ++c)
      if (lg[c] > mx) {
        mx = lg[c];
        arg = c;
      }
    float s = 0.f;
    for (int c = 0; c < 10; ++c) s += expf(lg[c] - mx);
    const float lse = mx + logf(s);
    for (int c = 0; c < 10; ++c) {
      const float lp = lg[c] - lse;
      if (logp_out) logp_out[c] = lp;
      if (TRAIN) {
        if (c == label) *rowloss = -lp;
        dl[c] = (expf(lp) - (c == label ? 1.0f : 0.0f)) * inv_rows;
      }
    }
    if (pred_out) *pred_out = arg;
  }
  if (!TRAIN) return;
  __syncthreads();

  // fc2 backward
  for (int e = tid; e < 500; e += DG_THREADS) {
    const int c = e / 50, j = e - c * 50;
    gout[G::F2W + e] = dl[c] * h1[j];
  }
  if (tid < 10) gout[G::F2B + tid] = dl[tid];
  if (tid < 50) {
    float s = 0.f;
    for (int c = 0; c < 10; ++c) s = fmaf(dl[c], par[G::F2W + c * 50 + tid], s);
    const float d = s * hm[tid];
    dh[tid] = d;
    gout[G::F1B + tid] = d;
  }
  __syncthreads();

  // fc1 backward: weights, then the pooled map's gradient through ReLU and Dropout2d
  for (int e = tid; e < 50 * FLAT; e += DG_THREADS) {
    const int j = e / FLAT, i = e - j * FLAT;
    gout[G::F1W + e] = dh[j] * a2[i];
  }
  for (int i = tid; i < FLAT; i += DG_THREADS) {
    float s = 0.f;
#pragma unroll 10
    for (int j = 0; j < 50; ++j) s = fmaf(dh[j], par[G::F1W + j * FLAT + i], s);
    const float md = drop_mul(k2d, row * 20u + (uint32_t)(i / PP2));
    g2[i] = a2[i] > 0.f ? s * md : 0.f;
  }
  __syncthreads();

  // conv2 backward: weights and bias ...
  for (int e = tid; e < G::NW2; e += DG_THREADS) {
    const int oc = e / 250, r = e - oc * 250, ic = r / 25, k = r - ic * 25, ky = k / 5, kx = k - ky * 5;
    const float* __restrict__ ap = a1 + ic * PP1 + ky * P1 + kx;
    float s = 0.f;
#pragma unroll 5
    for (int p = 0; p < PP2; ++p) {
      const int q = q2[oc * PP2 + p];
      s = fmaf(g2[oc * PP2 + p], ap[(q >> 8) * P1 + (q & 255)], s);
    }
    gout[G::W2 + e] = s;
  }
  if (tid < 20) {
    float s = 0.f;
    for (int p = 0; p < PP2; ++p) s += g2[tid * PP2 + p];
    gout[G::B2 + tid] = s;
  }
  // ... and its input's gradient through the first ReLU: a1[ic, y, x] feeds the maxima (oy, ox) with 0 <= y - oy < 5
  for (int o = tid; o < G::NA1; o += DG_THREADS) {
    const int ic = o / PP1, r = o - ic * PP1, y = r / P1, xx = r - y * P1;
    const int py0 = max(0, (y - 4) >> 1), py1 = min(P2 - 1, y >> 1);
    const int px0 = max(0, (xx - 4) >> 1), px1 = min(P2 - 1, xx >> 1);
    float s = 0.f;
#pragma unroll 1
    for (int oc = 0; oc < 20; ++oc) {
      const float* __restrict__ wp = w2s + (oc * 10 + ic) * 25;
      for (int py = py0; py <= py1; ++py)
        for (int px = px0; px <= px1; ++px) {
          const int p = oc * PP2 + py * P2 + px, q = q2[p];
          const int ky = y - (q >> 8), kx = xx - (q & 255);
          if ((unsigned)ky < 5u && (unsigned)kx < 5u) s = fmaf(g2[p], wp[ky * 5 + kx], s);
        }
    }
    g1[o] = a1[o] > 0.f ? s : 0.f;
  }
  __syncthreads();

  // conv1 backward: weights and bias
  for (int e = tid; e < G::NW1; e += DG_THREADS) {
    const int oc = e / (CIN * 25), r = e - oc * (CIN * 25), ic = r / 25, k = r - ic * 25, ky = k / 5, kx = k - ky * 5;
    const float* __restrict__ xp = xs + ic * H * H + ky * H + kx;
    float s = 0.f;
#pragma unroll 4
    for (int p = 0; p < PP1; ++p) {
      const int q = q1[oc * PP1 + p];
      s = fmaf(g1[oc * PP1 + p], xp[(q >> 8) * H + (q & 255)], s);
    }
    gout[G::W1 + e] = s;
  }
  if (tid >= DG_THREADS - 10) {
    const int oc = tid - (DG_THREADS - 10);
    float s = 0.f;
    for (int p = 0; p < PP1; ++p) s += g1[oc * PP1 + p];
    gout[G::B1 + oc] = s;
  }
}

// grid (rows, nets).  HIDDEN (eval only): `logp` is the (nets, N, 50) output of relu(fc1) and nothing else is written.
// TRAIN: row r of the minibatch is image ord[r] (or pos0 + r); its gradient goes to
// ws[(net * ws_rows + r) * stride ...], its loss to rowloss[net * ws_rows + r].  Eval: log-probs and prediction of image r.
template <bool TRAIN, bool HIDDEN = false>
__global__ __launch_bounds__(DG_THREADS) void digit_image_kernel(DigitTable tab, const float* __restrict__ state,
                                                                 int stride, const int* __restrict__ ord, int pos0,
                                                                 int rows, int ws_rows, uint32_t seed, long step, float p,
                                                                 float* __restrict__ ws, float* __restrict__ rowloss,
                                                                 float* __restrict__ logp, int* __restrict__ pred,
                                                                 long N) {
  __shared__ float lds[DG_LDS_FLOATS];
  const int net = blockIdx.y, r = blockIdx.x, kind = tab.kind[net];
  const float* par = state + (size_t)net * 3 * stride;
  const size_t img = TRAIN ? (size_t)(ord ? ord[r] : pos0 + r) : (size_t)r;
  DropKey k2d = {}, k1 = {};
  int label = 0;
  float* gout = nullptr;
  float* rl = nullptr;
  float* lp = nullptr;
  int* pr = nullptr;
  if (TRAIN) {
    k2d = digit_key(seed, kind, step, 0u, p);
    k1 = digit_key(seed, kind, step, 1u, p);
    label = tab.y[net][img];
    gout = ws + ((size_t)net * ws_rows + r) * stride;
    rl = rowloss + (size_t)net * ws_rows + r;
  } else if (HIDDEN) {
    float* hid = logp + ((size_t)net * N + r) * 50;
    if (kind == MMVAE_DIGIT_MNIST)
      digit_body<DigitM, false, true>(lds, par, tab.x[net] + img * DigitM::NX, 0, 1.0f, k2d, k1, (uint32_t)r, nullptr,
                                      nullptr, nullptr, nullptr, hid);
    else
      digit_body<DigitS, false, true>(lds, par, tab.x[net] + img * DigitS::NX, 0, 1.0f, k2d, k1, (uint32_t)r, nullptr,
                                      nullptr, nullptr, nullptr, hid);
    return;
  } else {
    lp = logp + ((size_t)net * N + r) * 10;
    pr = pred + (size_t)net * N + r;
  }
  const float inv_rows = 1.0f / (float)rows;
  if (kind == MMVAE_DIGIT_MNIST)
    digit_body<DigitM, TRAIN>(lds, par, tab.x[net] + img * DigitM::NX, label, inv_rows, k2d, k1, (uint32_t)r, gout, rl, lp,
                              pr);
  else
    digit_body<DigitS, TRAIN>(lds, par, tab.x[net] + img * DigitS::NX, label, inv_rows, k2d, k1, (uint32_t)r, gout, rl, lp,
                              pr);
}

// grid (ceil(stride / 64), nets), 256 threads: lane = parameter, wave w sums the rows [w R, (w + 1) R), R = ceil(rows / 4),
// in row order; the four partials are added as (0 + 1) + (2 + 3).  apply: torch.optim.Adam on state; else grad_out.
__global__ __launch_bounds__(DG_THREADS) void digit_fold_kernel(DigitTable tab, float* __restrict__ state, int stride,
                                                                const float* __restrict__ ws,
                                                                const float* __restrict__ rowloss, int rows, int ws_rows,
                                                                int apply, float step_size, float sq_bc2,
                                                                float* __restrict__ grad_out, float* __restrict__ loss_out,
                                                                int loss_stride) {
  __shared__ float part[4][64];
  const int net = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const int npar = tab.kind[net] == MMVAE_DIGIT_MNIST ? DigitM::NPAR : DigitS::NPAR;
  const int R = (rows + 3) >> 2, r0 = wave * R, r1 = min(rows, r0 + R);
  float s = 0.f;
  if (e < npar) {
    const float* __restrict__ src = ws + (size_t)net * ws_rows * stride + e;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) s += src[(size_t)r * stride];
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && e < npar) {
    const float g = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    if (apply) {
      float* st = state + (size_t)net * 3 * stride;
      const float b1 = 0.9f, b2 = 0.999f, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
      const float m = b1 * st[stride + e] + omb1 * g;
      const float v = b2 * st[2 * stride + e] + omb2 * (g * g);
      st[stride + e] = m;
      st[2 * stride + e] = v;
      const float denom = sqrtf(v) / sq_bc2 + eps;
      st[e] -= step_size * (m / denom);
    } else {
      grad_out[(size_t)net * stride + e] = g;
    }
  }
  if (loss_out && blockIdx.x == 0 && threadIdx.x == DG_THREADS - 1) {
    float l = 0.f;
    for (int r = 0; r < rows; ++r) l += rowloss[(size_t)net * ws_rows + r];
    loss_out[(size_t)net * loss_stride] = l / (float)rows;
  }
}

// grid (n_steps), any block: the masks of global step step0 + blockIdx.x as the image kernel draws them
__global__ void digit_masks_kernel(int kind, uint32_t seed, long step0, int batch, float p, float* __restrict__ m2d,
                                   float* __restrict__ m1) {
  const long t = step0 + blockIdx.x;
  const DropKey k2d = digit_key(seed, kind, t, 0u, p), k1 = digit_key(seed, kind, t, 1u, p);
  for (int i = threadIdx.x; i < batch * 20; i += blockDim.x) m2d[(size_t)blockIdx.x * batch * 20 + i] = drop_mul(k2d, (uint32_t)i);
  for (int i = threadIdx.x; i < batch * 50; i += blockDim.x) m1[(size_t)blockIdx.x * batch * 50 + i] = drop_mul(k1, (uint32_t)i);
}

// beta^t, t >= 1, by repeated squaring in double: the arithmetic mmvae_probe_train uses on the device
static double digit_powi(double b, long t) {
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

static int digit_table(const int* kinds, const float* const* images, const int* const* labels, int nets, int stride,
                       DigitTable* t) {
  if (nets < 1 || nets > MMVAE_DIGIT_MAX_NETS) return MMVAE_ERR_UNSUPPORTED;
  for (int i = 0; i < nets; ++i) {
    if (kinds[i] != MMVAE_DIGIT_MNIST && kinds[i] != MMVAE_DIGIT_SVHN) return MMVAE_ERR_UNSUPPORTED;
    if (stride < digit_npar(kinds[i])) return MMVAE_ERR_UNSUPPORTED;
    if (!images[i] || (labels && !labels[i])) return MMVAE_ERR_ARG;
    t->kind[i] = kinds[i];
    t->x[i] = images[i];
    t->y[i] = labels ? labels[i] : nullptr;
  }
  return MMVAE_OK;
}

extern "C" int mmvae_digit_n_params(int kind) {
  return kind == MMVAE_DIGIT_MNIST || kind == MMVAE_DIGIT_SVHN ? digit_npar(kind) : 0;
}

extern "C" size_t mmvae_digit_ws_floats(int nets, int batch, int stride) {
  return nets < 1 || batch < 1 || stride < 1 ? 0 : (size_t)nets * batch * ((size_t)stride + 1);
}

extern "C" int mmvae_digit_eval(const float* state, const int* kinds, const float* const* images, float* logp, int* pred,
                                int nets, int stride, long N, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && kinds && images && logp && pred && N > 0);
  if (N > 0x7FFFFFFFl) return MMVAE_ERR_UNSUPPORTED;
  DigitTable t = {};
  const int rc = digit_table(kinds, images, nullptr, nets, stride, &t);
  if (rc != MMVAE_OK) return rc;
  hipLaunchKernelGGL(digit_image_kernel<false>, dim3((unsigned)N, nets), dim3(DG_THREADS), 0, (hipStream_t)stream, t, state,
                     stride, (const int*)nullptr, 0, 1, 0, 0u, 0l, 0.f, (float*)nullptr, (float*)nullptr, logp, pred, N);
  return mmvae_launch_status();
}

extern "C" int mmvae_digit_hidden(const float* state, const int* kinds, const float* const* images, float* hidden,
                                  int nets, int stride, long N, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && kinds && images && hidden && N > 0);
  if (N > 0x7FFFFFFFl) return MMVAE_ERR_UNSUPPORTED;
  DigitTable t = {};
  const int rc = digit_table(kinds, images, nullptr, nets, stride, &t);
  if (rc != MMVAE_OK) return rc;
  hipLaunchKernelGGL((digit_image_kernel<false, true>), dim3((unsigned)N, nets), dim3(DG_THREADS), 0, (hipStream_t)stream,
                     t, state, stride, (const int*)nullptr, 0, 1, 0, 0u, 0l, 0.f, (float*)nullptr, (float*)nullptr, hidden,
                     (int*)nullptr, N);
  return mmvae_launch_status();
}

extern "C" int mmvae_digit_grad(const float* state, const int* kinds, const float* const* images,
                                const int* const* labels, float* ws, float* grad, float* rowloss, int nets, int stride,
                                int rows, uint32_t seed, long step, float p, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && kinds && images && labels && ws && grad && rowloss && rows > 0 && step >= 0);
  // rows <= 65535: a budget for ws (one gradient row of `stride` floats per image: 8.2 GB per network there), no index limit
  if (!(p >= 0.f && p < 1.f) || rows > 65535) return MMVAE_ERR_UNSUPPORTED;
  DigitTable t = {};
  const int rc = digit_table(kinds, images, labels, nets, stride, &t);
  if (rc != MMVAE_OK) return rc;
  hipLaunchKernelGGL(digit_image_kernel<true>, dim3(rows, nets), dim3(DG_THREADS), 0, (hipStream_t)stream, t, state, stride,
                     (const int*)nullptr, 0, rows, rows, seed, step, p, ws, rowloss, (float*)nullptr, (int*)nullptr, 0l);
  hipLaunchKernelGGL(digit_fold_kernel, dim3((stride + 63) / 64, nets), dim3(DG_THREADS), 0, (hipStream_t)stream, t,
                     (float*)nullptr, stride, ws, rowloss, rows, rows, 0, 0.f, 0.f, grad, (float*)nullptr, 0);
  return mmvae_launch_status();
}

extern "C" int mmvae_digit_train(float* state, const int* kinds, const float* const* images, const int* const* labels,
                                 const int* order, int order_epochs, float* ws, float* loss, int nets, int stride, int N,
                                 int batch, long step0, int n_steps, float lr, uint32_t seed, float p,
                                 mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(state && kinds && images && labels && ws && loss && N > 0 && step0 >= 0 && n_steps > 0);
  if (batch < 1 || batch > 65535 || !(p >= 0.f && p < 1.f)) return MMVAE_ERR_UNSUPPORTED;
  DigitTable t = {};
  const int rc = digit_table(kinds, images, labels, nets, stride, &t);
  if (rc != MMVAE_OK) return rc;
  const long spe = ((long)N + batch - 1) / batch;
  if (order) MMVAE_CHECK_ARG((step0 + n_steps - 1) / spe < order_epochs);
  float* rowloss = ws + (size_t)nets * batch * stride;
  for (int k = 0; k < n_steps; ++k) {
    const long step = step0 + k, epoch = step / spe;
    const int b0 = (int)(step - epoch * spe) * batch, rows = min(batch, N - b0);
    const int* ord = order ? order + (size_t)epoch * N + b0 : nullptr;
    const double bc1 = 1.0 - digit_powi(0.9, step + 1), bc2 = 1.0 - digit_powi(0.999, step + 1);
    hipLaunchKernelGGL(digit_image_kernel<true>, dim3(rows, nets), dim3(DG_THREADS), 0, (hipStream_t)stream, t, state,
                       stride, ord, b0, rows, batch, seed, step, p, ws, rowloss, (float*)nullptr, (int*)nullptr, 0l);
    hipLaunchKernelGGL(digit_fold_kernel, dim3((stride + 63) / 64, nets), dim3(DG_THREADS), 0, (hipStream_t)stream, t,
                       state, stride, ws, rowloss, rows, batch, 1, (float)((double)lr / bc1), (float)sqrt(bc2),
                       (float*)nullptr, loss + k, n_steps);
  }
  return mmvae_launch_status();
}

extern "C" int mmvae_digit_masks(float* m2d, float* m1, int kind, uint32_t seed, long step0, int n_steps, int batch,
                                 float p, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(m2d && m1 && step0 >= 0 && n_steps > 0);
  if ((kind != MMVAE_DIGIT_MNIST && kind != MMVAE_DIGIT_SVHN) || batch < 1 || batch > 65535 || !(p >= 0.f && p < 1.f))
    return MMVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(digit_masks_kernel, dim3(n_steps), dim3(DG_THREADS), 0, (hipStream_t)stream, kind, seed, step0, batch,
                     p, m2d, m1);
  return mmvae_launch_status();
}
