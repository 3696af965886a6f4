// Image reconstruction quality (ops.image_quality): per pair of images the mean squared and mean absolute
// error, PSNR, SSIM (Wang et al. 2004) and the multi-scale values, in float64 from fp32 planes.  One launch, one workgroup of
// 256 threads per image pair: the channel means and the multi-scale powers stay in the launch, nothing but the (N, 5 + S)
// result is written, no atomics, every sum in one fixed order (an image's bits do not depend on its neighbours in the launch).
//
// Per plane: the fp32 plane pair is staged in LDS (the squared and absolute differences ride in that pass).  Per level the five
// products x, y, x^2, y^2, xy are filtered horizontally into a ring of win - 1 + rs rows (rs = 256 / valid columns input rows per
// step, so that every thread owns one (row, column) of a step), then vertically from the ring; a position's l and cs are
// formed in registers and summed per thread in step order, then over the lanes (butterfly) and the four waves in order.  The
// next level is pooled 2 x 2 in double from the level before it, the levels alternating between the two plane regions.
// LDS: 512 B + 8 HW' (level 0 as fp32; later level 2) + 4 HW' (level 1; later level 3) + the ring, HW' = 64 x 64 or, for planes
// with both sides <= 32, 32 x 32: 79.6 KiB at most (two workgroups per CU), 31.1 KiB for the small class (five).
#include <math.h>

#include "common.hpp"

#define IQ_THREADS 256
#define IQ_MAPS 5

struct IqArgs {
  const float* x;
  const float* y;
  double* out;
  int C, H, W, S;
  double g[MMVAE_IQ_MAX_WIN];          // the window's 1-D weights (their outer product is the 2-D window)
  double msw[MMVAE_IQ_MAX_SCALES];     // the multi-scale exponents
  double c1, c2, f, range2;
};

// sums over the block, in thread 0 only: lanes by butterfly, then the waves in order.  `red`: 4 x IQ_MAPS doubles
template <int K>
__device__ __forceinline__ void iq_block_sum(double (&v)[K], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave * IQ_MAPS + k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[IQ_MAPS + k]) + red[2 * IQ_MAPS + k]) + red[3 * IQ_MAPS + k];
}

// one level of one plane pair sx, sy (h, w) in LDS: acc += per-thread sums of (l cs, cs, l) over the valid positions
template <int WIN, typename T>
__device__ __forceinline__ void iq_level(const T* sx, const T* sy, int h, int w, const IqArgs& a, double* ring, double (&acc)[3]) {
  const int tid = threadIdx.x;
  const int ow = w - WIN + 1;
  int rs = IQ_THREADS / ow;      // input rows per step
  if (rs > h) rs = h;
  const int ring_rows = WIN - 1 + rs;
  const int rr = tid / ow, col = tid - rr * ow;
  const bool mine = rr < rs;
  for (int r0 = 0; r0 < h; r0 += rs) {
    const int r = r0 + rr;
    const bool live = mine && r < h;
    if (live) {
      const T* px = sx + r * w + col;
      const T* py = sy + r * w + col;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const double xv = (double)px[k], yv = (double)py[k], gk = a.g[k];
        s0 += gk * xv;
        s1 += gk * yv;
        s2 += gk * (xv * xv);
        s3 += gk * (yv * yv);
        s4 += gk * (xv * yv);
      }
      double* q = ring + (r % ring_rows) * IQ_MAPS * ow + col;
      q[0] = s0;
      q[ow] = s1;
      q[2 * ow] = s2;
      q[3 * ow] = s3;
      q[4 * ow] = s4;
    }
    __syncthreads();
    const int o = r - (WIN - 1);      // the output row whose last input row is r
    if (live && o >= 0) {
      int slot = o % ring_rows;
      double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
      for (int i = 0; i < WIN; ++i) {
        const double* q = ring + slot * IQ_MAPS * ow + col;
        const double gi = a.g[i];
        mx += gi * q[0];
        my += gi * q[ow];
        xx += gi * q[2 * ow];
        yy += gi * q[3 * ow];
        xy += gi * q[4 * ow];
        slot = slot + 1 == ring_rows ? 0 : slot + 1;
      }
      const double vx = a.f * (xx - mx * mx), vy = a.f * (yy - my * my), cxy = a.f * (xy - mx * my);
      const double l = (2.0 * mx * my + a.c1) / (mx * mx + my * my + a.c1);
      const double cs = (2.0 * cxy + a.c2) / (vx + vy + a.c2);
      acc[0] += l * cs;
      acc[1] += cs;
      acc[2] += l;
    }
    __syncthreads();      // the next step writes the slots of rows this step has read
  }
}

// 2 x 2 average pooling of the plane pair src (h, w) into dst (h / 2, w / 2), in double
template <typename T>
__device__ __forceinline__ void iq_pool(const T* src, double* dst, int h, int w) {
  const int h2 = h >> 1, w2 = w >> 1, n2 = h2 * w2;
  for (int i = threadIdx.x; i < n2; i += IQ_THREADS) {
    const int r = i / w2, c = i - r * w2;
    const T* p = src + 2 * r * w + 2 * c;
    const T* q = p + h * w;
    dst[i] = 0.25 * (((double)p[0] + (double)p[1]) + ((double)p[w] + (double)p[w + 1]));
    dst[n2 + i] = 0.25 * (((double)q[0] + (double)q[1]) + ((double)q[w] + (double)q[w + 1]));
  }
  __syncthreads();
}

// grid N, 256 threads.  SIDE = 64, or 32 for planes with both sides <= 32 (less LDS, more workgroups per CU)
template <int WIN, int SIDE>
__global__ __launch_bounds__(IQ_THREADS) void iq_kernel(const IqArgs a) {
  constexpr int P0 = SIDE * SIDE;                                              // doubles: 2 planes of fp32, SIDE x SIDE
  constexpr int P1 = SIDE * SIDE / 2;                                          // doubles: 2 planes (SIDE / 2)^2
  constexpr int RING = ((WIN - 1) * (SIDE + 1 - WIN) + IQ_THREADS) * IQ_MAPS;  // >= (WIN - 1 + rs) ow maps, rs ow <= 256
  __shared__ double lds[64 + P0 + P1 + RING];
  double* red = lds;            // [4][IQ_MAPS]
  double* lv = lds + 32;        // [S][3]: the levels' (ssim, cs, l), summed over the channels by thread 0
  double* p0d = lds + 64;
  float* p0f = reinterpret_cast<float*>(p0d);
  double* p1d = p0d + P0;
  double* ring = p1d + P1;
  const int tid = threadIdx.x;
  const long n = blockIdx.x;
  const int HW = a.H * a.W;
  if (tid < 3 * MMVAE_IQ_MAX_SCALES) lv[tid] = 0.0;
  double se = 0.0, ae = 0.0;
  for (int c = 0; c < a.C; ++c) {
    const float* gx = a.x + (n * a.C + c) * (long)HW;
    const float* gy = a.y + (n * a.C + c) * (long)HW;
    double d2[2] = {0.0, 0.0};
    for (int i = tid; i < HW; i += IQ_THREADS) {
      const float xv = gx[i], yv = gy[i];
      p0f[i] = xv;
      p0f[HW + i] = yv;
      const double d = (double)xv - (double)yv;
      d2[0] += d * d;
      d2[1] += fabs(d);
    }
    iq_block_sum<2>(d2, red);      // (its barriers also publish the staged planes)
    if (tid == 0) {
      se += d2[0];
      ae += d2[1];
    }
    int h = a.H, w = a.W;
    for (int s = 0; s < a.S; ++s) {
      double acc[3] = {0.0, 0.0, 0.0};
      const double* lvl = (s & 1) ? p1d : p0d;
      if (s == 0)
        iq_level<WIN, float>(p0f, p0f + HW, h, w, a, ring, acc);
      else
        iq_level<WIN, double>(lvl, lvl + h * w, h, w, a, ring, acc);
      iq_block_sum<3>(acc, red);
      if (tid == 0) {
        const double positions = (double)((h - WIN + 1) * (w - WIN + 1));
        lv[3 * s] += acc[0] / positions;
        lv[3 * s + 1] += acc[1] / positions;
        lv[3 * s + 2] += acc[2] / positions;
      }
      if (s + 1 < a.S) {
        double* next = (s & 1) ? p0d : p1d;
        if (s == 0)
          iq_pool<float>(p0f, next, h, w);
        else
          iq_pool<double>(lvl, next, h, w);
        h >>= 1;
        w >>= 1;
      }
    }
  }
  if (tid == 0) {
    double* o = a.out + n * (5 + a.S);
    const double count = (double)a.C * (double)HW, ch = (double)a.C;
    const double mse = se / count, ssim = lv[0] / ch;
    o[0] = mse;
    o[1] = ae / count;
    o[2] = mse > 0.0 ? 10.0 * log10(a.range2 / mse) : (double)INFINITY;
    o[3] = ssim;
    double ms;
    if (a.S == 1) {
      ms = fmax(ssim, 0.0);
      o[5] = lv[2] / ch;
    } else {
      ms = 1.0;
      for (int s = 0; s < a.S; ++s) {
        const double v = lv[3 * s + (s + 1 < a.S ? 1 : 2)] / ch;      // cs of every level but the last, l of the last
        o[5 + s] = v;
        ms *= pow(fmax(v, 0.0), a.msw[s]);
      }
    }
    o[4] = ms;
  }
}

static bool iq_plane_ok(int H, int W, int win) {
  return win >= MMVAE_IQ_MIN_WIN && win <= MMVAE_IQ_MAX_WIN && (win & 1) && H >= win && W >= win && H <= MMVAE_IQ_MAX_SIDE &&
         W <= MMVAE_IQ_MAX_SIDE;
}

extern "C" int mmvae_image_quality_max_scales(int H, int W, int win) {
  if (!iq_plane_ok(H, W, win)) return 0;
  int s = 1;
  while (s < MMVAE_IQ_MAX_SCALES && H % 2 == 0 && W % 2 == 0 && H / 2 >= win && W / 2 >= win) {
    H /= 2;
    W /= 2;
    ++s;
  }
  return s;
}

extern "C" size_t mmvae_image_quality_lds_bytes(int H, int W, int win) {
  if (!iq_plane_ok(H, W, win)) return 0;
  const int side = (H <= 32 && W <= 32) ? 32 : 64;
  return sizeof(double) * (size_t)(64 + side * side + side * side / 2 + ((win - 1) * (side + 1 - win) + IQ_THREADS) * IQ_MAPS);
}

template <int WIN>
static void iq_launch(const IqArgs& a, long N, hipStream_t s) {
  if (a.H <= 32 && a.W <= 32)
    hipLaunchKernelGGL((iq_kernel<WIN, 32>), dim3((unsigned)N), dim3(IQ_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((iq_kernel<WIN, 64>), dim3((unsigned)N), dim3(IQ_THREADS), 0, s, a);
}

extern "C" int mmvae_image_quality(const float* x, const float* y, double* out, long N, int C, int H, int W, int win,
                                   const double* window, double data_range, double c1, double c2, double cov_scale, int scales,
                                   const double* ms_weights, mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(x && y && out && window && (scales == 1 || ms_weights));
  if (N < 1 || N > MMVAE_IQ_MAX_ROWS || C < 1 || C > MMVAE_IQ_MAX_CHANNELS || scales < 1 ||
      scales > mmvae_image_quality_max_scales(H, W, win))
    return MMVAE_ERR_UNSUPPORTED;
  IqArgs a;
  a.x = x;
  a.y = y;
  a.out = out;
  a.C = C;
  a.H = H;
  a.W = W;
  a.S = scales;
  for (int i = 0; i < MMVAE_IQ_MAX_WIN; ++i) a.g[i] = i < win ? window[i] : 0.0;
  for (int i = 0; i < MMVAE_IQ_MAX_SCALES; ++i) a.msw[i] = (scales > 1 && i < scales) ? ms_weights[i] : 0.0;
  a.c1 = c1;
  a.c2 = c2;
  a.f = cov_scale;
  a.range2 = data_range * data_range;
  hipStream_t s = (hipStream_t)stream;
  switch (win) {
    case 3: iq_launch<3>(a, N, s); break;
    case 5: iq_launch<5>(a, N, s); break;
    case 7: iq_launch<7>(a, N, s); break;
    case 9: iq_launch<9>(a, N, s); break;
    default: iq_launch<11>(a, N, s); break;
  }
  return mmvae_launch_status();
}
