// Text generation quality (ops.text_quality): per pair of a hypothesis (the decoder's logits, or token ids)
// and a reference (token ids) the position matches, the Levenshtein distance, the longest common subsequence, the clipped
// n-gram matches of orders 1 .. 4 (BLEU's counts) -- over tokens and, with a separator, over words -- and the reference's
// negative log-likelihood under the logits in float64.  One launch, one wave (a workgroup of 64 threads) per pair: nothing
// but the pair's outputs is written, no atomics, the one float sum in one fixed order, so a pair's bits depend on nothing else.
//
// LDS holds the two sequences, the word table and the two word-id sequences (4160 B).  The two DP tables never exist: lane l
// owns the columns 4 l + 1 .. 4 l + 4 of both and walks the rows one step behind lane l - 1, which hands it the row's value
// at column 4 l by a shuffle (La + ceil(Lb / 4) - 1 steps of 4 cells).  The n-gram pass gives every lane a position p of the
// hypothesis and counts, for all orders at once (an order-n match is an order-(n - 1) match whose next token agrees), the
// earlier positions of the hypothesis and the positions of the reference that hold the same n-gram: p is the k-th occurrence
// (from 0) of its n-gram and counts iff k < the reference's count, which sums to Papineni's clipped count.
#include <math.h>

#include "common.hpp"

#define TQ_T MMVAE_TQ_MAX_STEPS
#define TQ_PAD (TQ_T + 4)      // a sequence and what a 4-gram window reads past its end
#define TQ_WPAD (TQ_T / 2 + 4) // at most T / 2 words of a sequence
#define TQ_HYP_PAD -1          // past the hypothesis' end, -2 past the reference's: no token, and different from each other
#define TQ_REF_PAD -2
#define TQ_TOK_OUT 13          // hyp_len, ref_len, same, edit, lcs, match[4], total[4]
#define TQ_WORD_OUT 12         // hyp_len, ref_len, edit, lcs, match[4], total[4]

struct TqArgs {
  const float* logits;
  const int* hyp;
  const int* ref;
  const int* ref_len;
  const int* hyp_len;
  int* pred;
  int* tok;
  int* word;
  double* nll;
  int* nll_steps;
  int Th, Tr, V, eos, trim, sep, K;
};

__device__ __forceinline__ int tq_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int tq_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int tq_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// the length of s[0 .. L) cut before its first `eos`, then without its trailing `trim`s (either < 0: none)
__device__ __forceinline__ int tq_cut(const int* s, int L, int eos, int trim, int lane) {
  if (eos >= 0) {
    int first = L;
    for (int t = lane; t < L; t += 64)
      if (s[t] == eos) first = min(first, t);
    L = tq_min(first);
  }
  if (trim >= 0) {
    int last = 0;
    for (int t = lane; t < L; t += 64)
      if (s[t] != trim) last = t + 1;
    L = tq_max(last);
  }
  return L;
}

// Levenshtein distance and LCS length of a[0 .. La) and b[0 .. Lb), in every lane.  Rows i = 1 .. La are a's tokens, columns
// j = 1 .. Lb b's; lane l owns the columns 4 l + 1 .. 4 l + 4 and computes row s - l at step s.
__device__ __forceinline__ void tq_align(const int* a, int La, const int* b, int Lb, int lane, int& edit, int& lcs) {
  if (La == 0 || Lb == 0) {
    edit = max(La, Lb);
    lcs = 0;
    return;
  }
  const int nl = (Lb + 3) >> 2;      // the lanes that own a column
  int bj[4], ue[4], uc[4];           // the columns' tokens; row i - 1 of the two tables at these columns
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = 4 * lane + c;
    bj[c] = j < Lb ? b[j] : TQ_REF_PAD;
    ue[c] = j + 1;
    uc[c] = 0;
  }
  int pe = 4 * lane, pc = 0;          // row i - 1 at column 4 l
  int last_e = 0, last_c = 0;         // the row just computed at column 4 l + 4
  for (int s = 1; s < La + nl; ++s) {
    int re = __shfl_up(last_e, 1, 64), rc = __shfl_up(last_c, 1, 64);      // row i at column 4 l: lane l - 1's last step
    const int i = s - lane;
    if (lane == 0) {
      re = i;
      rc = 0;
    }
    if (i >= 1 && i <= La && lane < nl) {
      const int ai = a[i - 1];
      int le = re, lc = rc, de = pe, dc = pc;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool eq = ai == bj[c];
        const int e = min(min(ue[c], le) + 1, de + (eq ? 0 : 1));
        const int l = eq ? dc + 1 : max(uc[c], lc);
        de = ue[c];
        dc = uc[c];
        ue[c] = e;
        uc[c] = l;
        le = e;
        lc = l;
      }
      pe = re;
      pc = rc;
      last_e = le;
      last_c = lc;
    }
  }
  const int c = (Lb - 1) & 3;
  const int ve = c == 0 ? ue[0] : c == 1 ? ue[1] : c == 2 ? ue[2] : ue[3];
  const int vc = c == 0 ? uc[0] : c == 1 ? uc[1] : c == 2 ? uc[2] : uc[3];
  edit = __shfl(ve, (Lb - 1) >> 2, 64);
  lcs = __shfl(vc, (Lb - 1) >> 2, 64);
}

// k[n] += the positions q of x[0 .. Lx) (UPTO: only q < p) whose (n + 1)-gram equals hp[0 .. n]; x is padded past its end
template <bool UPTO>
__device__ __forceinline__ void tq_count(const int* x, int Lx, const int (&hp)[4], int p, int (&k)[4]) {
  int x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
#pragma unroll 1      // (unrolled further, the compare masks of the copies run the kernel out of scalar registers)
  for (int q = 0; q < Lx; ++q) {      // (x[q + 4] <= x[TQ_PAD - 1]: every lane reads the same word)
    // (bitwise, not short-circuit: four compares and four adds per position, no branch)
    const int e0 = (int)(x0 == hp[0]) & (int)(!UPTO || q < p);
    const int e1 = e0 & (int)(x1 == hp[1]);
    const int e2 = e1 & (int)(x2 == hp[2]);
    const int e3 = e2 & (int)(x3 == hp[3]);
    k[0] += e0;
    k[1] += e1;
    k[2] += e2;
    k[3] += e3;
    x0 = x1;
    x1 = x2;
    x2 = x3;
    x3 = x[q + 4];
  }
}

// the counts of one level: a (hypothesis, padded with TQ_HYP_PAD) against b (reference, padded with TQ_REF_PAD).
// out (lane 0): La, Lb, [same,] edit, lcs, match[4], total[4]
template <bool SAME>
__device__ __forceinline__ void tq_level(const int* a, int La, const int* b, int Lb, int K, int lane, int* out) {
  int same = 0;
  if (SAME) {
    const int L = min(La, Lb);
    for (int t = lane; t < L; t += 64) same += a[t] == b[t];
    same = tq_sum(same);
  }
  int edit, lcs;
  tq_align(a, La, b, Lb, lane, edit, lcs);
  int m[4] = {0, 0, 0, 0};
#pragma unroll 1
  for (int p0 = 0; p0 < La; p0 += 64) {
    const int p = p0 + lane;      // (<= 255: p + 3 is inside the array; past La + 2 it holds anything, and `left` gates it)
    const int hp[4] = {a[p], a[p + 1], a[p + 2], a[p + 3]};
    int k[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0};
    tq_count<true>(a, min(p0 + 64, La), hp, p, k);
    tq_count<false>(b, Lb, hp, p, c);
    const int left = La - p;      // the orders that fit at p
#pragma unroll
    for (int n = 0; n < 4; ++n) m[n] += (n < K && left > n && k[n] < c[n]);
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) m[n] = tq_sum(m[n]);
  if (lane == 0) {
    int* o = out;
    *o++ = La;
    *o++ = Lb;
    if (SAME) *o++ = same;
    *o++ = edit;
    *o++ = lcs;
#pragma unroll
    for (int n = 0; n < 4; ++n) o[n] = m[n];
#pragma unroll
    for (int n = 0; n < 4; ++n) o[4 + n] = n < K ? max(La - n, 0) : 0;
  }
}

// the words (maximal runs of tokens != sep) of s[0 .. L), appended to the table at `count`: start (s at `base` of the token
// array) and length.  -> the table's new size
__device__ __forceinline__ int tq_words(const int* s, int base, int L, int sep, int count, unsigned short* wst,
                                        unsigned short* wln, int lane) {
  for (int t0 = 0; t0 < L; t0 += 64) {
    const int t = t0 + lane;
    const bool start = t < L && s[t] != sep && (t == 0 || s[t - 1] == sep);
    const unsigned long long starts = __ballot(start);
    if (start) {
      const int w = count + __popcll(starts & ((1ull << lane) - 1ull));
      int e = t + 1;
      while (e < L && s[e] != sep) ++e;
      wst[w] = (unsigned short)(base + t);
      wln[w] = (unsigned short)(e - t);
    }
    count += __popcll(starts);
  }
  return count;
}

// grid N, 64 threads: one wave per pair
__global__ __launch_bounds__(64) void tq_kernel(const TqArgs a) {
  __shared__ int tok[2 * TQ_PAD];       // the reference at 0, the hypothesis at TQ_PAD
  __shared__ int wid[2 * TQ_WPAD];      // their words' ids
  __shared__ unsigned short wst[TQ_T], wln[TQ_T];
  int* sr = tok;
  int* sh = tok + TQ_PAD;
  const int lane = threadIdx.x;
  const size_t n = blockIdx.x;
  const int Th = a.Th, Tr = a.Tr, V = a.V;
  const int ref_len = min(max(a.ref_len[n], 0), Tr);
  const int hyp_len = a.hyp_len ? min(max(a.hyp_len[n], 0), Th) : Th;
  const int* ref = a.ref + n * Tr;
  for (int t = lane; t < Tr; t += 64) sr[t] = ref[t];
  if (a.logits) {
    // lane t decodes step t: the first maximum, and the step's term of the negative log-likelihood in double, v rising
    const int S = min(ref_len, Th);
    double part = 0.0;
    for (int t = lane; t < Th; t += 64) {
      const float* row = a.logits + (n * Th + t) * V;
      float bv = row[0];
      int bi = 0;
      for (int v = 1; v < V; ++v) {
        const float x = row[v];
        if (x > bv) {
          bv = x;
          bi = v;
        }
      }
      sh[t] = bi;
      a.pred[n * Th + t] = bi;
      if (t < S) {
        const double m = (double)bv;
        double s = 0.0;
        for (int v = 0; v < V; ++v) s += exp((double)row[v] - m);
        part += (m + log(s)) - (double)row[min(max(ref[t], 0), V - 1)];      // (ids outside [0, V) are the caller's to refuse)
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);      // the lanes' sums (each over t rising) by butterfly
    if (lane == 0) {
      a.nll[n] = part;
      a.nll_steps[n] = S;
    }
  } else {
    const int* hyp = a.hyp + n * Th;
    for (int t = lane; t < Th; t += 64) sh[t] = hyp[t];
  }
  __syncthreads();
  const int Lr = tq_cut(sr, ref_len, a.eos, a.trim, lane);
  const int Lh = tq_cut(sh, hyp_len, a.eos, a.trim, lane);
  __syncthreads();
  if (lane < 3) {
    sr[Lr + lane] = TQ_REF_PAD;
    sh[Lh + lane] = TQ_HYP_PAD;
  }
  __syncthreads();
  tq_level<true>(sh, Lh, sr, Lr, a.K, lane, a.tok + n * TQ_TOK_OUT);
  if (a.sep < 0) return;
  // words: the table lists the reference's, then the hypothesis'; a word's id is the index of the first equal word in it
  const int nr = tq_words(sr, 0, Lr, a.sep, 0, wst, wln, lane);
  const int nw = tq_words(sh, TQ_PAD, Lh, a.sep, nr, wst, wln, lane);
  const int nh = nw - nr;
  int* wr = wid;
  int* wh = wid + TQ_WPAD;
  __syncthreads();
  for (int w = lane; w < nw; w += 64) {
    const int st = wst[w], ln = wln[w];
    int id = w;
    for (int u = 0; u < w; ++u) {
      if (wln[u] != ln) continue;
      const int su = wst[u];
      int j = 0;
      while (j < ln && tok[su + j] == tok[st + j]) ++j;
      if (j == ln) {
        id = u;
        break;
      }
    }
    if (w < nr)
      wr[w] = id;
    else
      wh[w - nr] = id;
  }
  if (lane < 3) {
    wr[nr + lane] = TQ_REF_PAD;
    wh[nh + lane] = TQ_HYP_PAD;
  }
  __syncthreads();
  tq_level<false>(wh, nh, wr, nr, a.K, lane, a.word + n * TQ_WORD_OUT);
}

extern "C" size_t mmvae_text_quality_lds_bytes(int Th, int Tr) {
  if (Th < 1 || Th > MMVAE_TQ_MAX_STEPS || Tr < 1 || Tr > MMVAE_TQ_MAX_STEPS) return 0;
  return sizeof(int) * (2 * TQ_PAD + 2 * TQ_WPAD) + sizeof(unsigned short) * 2 * TQ_T;
}

extern "C" int mmvae_text_quality(const float* logits, const int* hyp_ids, const int* ref_ids, const int* ref_lengths,
                                  const int* hyp_lengths, int* pred, int* token_out, int* word_out, double* nll,
                                  int* nll_steps, long N, int Th, int Tr, int V, int eos, int trim, int sep, int max_order,
                                  mmvae_stream_t stream) {
  MMVAE_CHECK_ARG(ref_ids && ref_lengths && token_out && (logits ? (pred && nll && nll_steps) : hyp_ids != nullptr) &&
                  (sep < 0 ? word_out == nullptr : word_out != nullptr));
  if (N < 1 || N > MMVAE_TQ_MAX_ROWS || Th < 1 || Th > MMVAE_TQ_MAX_STEPS || Tr < 1 || Tr > MMVAE_TQ_MAX_STEPS || V < 2 ||
      V > MMVAE_TQ_MAX_VOCAB || max_order < 1 || max_order > MMVAE_TQ_MAX_ORDER)
    return MMVAE_ERR_UNSUPPORTED;
  TqArgs a;
  a.logits = logits;
  a.hyp = hyp_ids;
  a.ref = ref_ids;
  a.ref_len = ref_lengths;
  a.hyp_len = hyp_lengths;
  a.pred = pred;
  a.tok = token_out;
  a.word = word_out;
  a.nll = nll;
  a.nll_steps = nll_steps;
  a.Th = Th;
  a.Tr = Tr;
  a.V = V;
  a.eos = eos < 0 ? -1 : eos;
  a.trim = trim < 0 ? -1 : trim;
  a.sep = sep < 0 ? -1 : sep;
  a.K = max_order;
  hipLaunchKernelGGL(tq_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, a);
  return mmvae_launch_status();
}
