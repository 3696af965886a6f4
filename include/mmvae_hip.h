/*
 * mmvae_hip.h — C ABI of the MI355X (gfx950) hot-path library for the multimodal-VAE training step.
 *
 * The reference (gabinsane/multimodal-vae-comparison) has no native code and no FFI: every "kernel" it
 * runs is a stock PyTorch op reached through torch.nn.  The entry points below are the op
 * sequences of its per-step path, each citing the reference lines it replaces.  Paths are
 * relative to /root/reference/multimodal_compare/.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated; no torch types, no allocation,
 *     no host synchronisation; every call only enqueues work on `stream` (graph-capturable, re-entrant
 *     per stream);
 *   - return value: 0 = ok, MMVAE_ERR_* otherwise (the Python binding raises RuntimeError);
 *   - `ws` = caller-provided workspace; the number of floats needed is returned by the matching
 *     *_ws_floats() query (0 => may be NULL);
 *   - `accumulate` != 0: results are ADDED to the destination (gradient accumulation into a flat grad
 *     buffer), else they overwrite it.
 */
#ifndef MMVAE_HIP_H
#define MMVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mmvae_stream_t; /* hipStream_t */

enum {
  MMVAE_OK = 0,
  MMVAE_ERR_ARG = 1,         /* null pointer / non-positive size */
  MMVAE_ERR_UNSUPPORTED = 2, /* shape outside what the kernels are built for */
  MMVAE_ERR_LAUNCH = 3,      /* hipGetLastError() != hipSuccess after launch */
  MMVAE_ERR_NO_CONVERGENCE = 4 /* an iteration reached its cap (mmvae_sym_eig: MMVAE_EIG_MAX_SWEEPS sweeps) */
};

/* input transform applied to an operand while it is staged into LDS */
enum { MMVAE_ACT_NONE = 0, MMVAE_ACT_SILU = 1, MMVAE_ACT_RELU = 2, MMVAE_ACT_GELU = 3 };
/* epilogue applied to the accumulator before the store; `aux` has the output's shape */
enum {
  MMVAE_EP_NONE = 0,
  MMVAE_EP_RELU = 1,          /* y = max(acc + bias, 0)                                           */
  MMVAE_EP_MUL_RELU_MASK = 2, /* y = acc * (aux > 0)        (dgrad through a ReLU, aux = saved u or y) */
  MMVAE_EP_MUL_SILU_GRAD = 3, /* y = acc * silu'(aux)       (dgrad through a SiLU, aux = saved u)   */
  MMVAE_EP_GELU = 4,          /* y = gelu(acc + bias); aux (if non-null) RECEIVES acc + bias        */
  MMVAE_EP_MUL_GELU_GRAD = 5, /* y = acc * gelu'(aux)                                              */
  MMVAE_EP_SIGMOID_CLAMP = 6, /* y = clamp(sigmoid(acc + bias), 1e-6, 1 - 1e-6)  (Dec_CNN, decoders.py:96-97) */
  MMVAE_EP_SIGMOID = 7,       /* y = sigmoid(acc + bias)                          (Dec_SVHN, decoders.py:144) */
  MMVAE_EP_ADD_AUX = 8        /* y = acc + bias + aux   (dgrad of a sub-layer's first op + the residual branch's gradient) */
};

/* Inverted dropout (train mode of the text towers: nn.Dropout(0.1) in PositionalEncoding and in every
 * Transformer sub-layer, models/encoders.py:790, decoders.py:669).  Counter-based: element i of site `site` is kept
 * iff hash(seed, counter, site, i) >= p, so the backward kernels regenerate the mask instead of storing it.
 * state[0] = seed, state[1] = running counter, state[2 + slot] = the counter value of forward call `slot` of this
 * step (mmvae_dropout_advance bumps the counter and fills the slot; forward and backward of that call read it).
 * A NULL pointer / p == 0 disables dropout.  Philox streams of the reference cannot be matched bit for bit; parity
 * under dropout is tested with the masks extracted by mmvae_dropout_mask and fed to the oracle. */
typedef struct {
  const uint32_t* state;
  uint32_t slot;
  uint32_t site;
  float p;
} mmvae_dropout_t;
#define MMVAE_DROPOUT_SLOTS 16
int mmvae_dropout_advance(uint32_t* state, uint32_t slot, mmvae_stream_t stream);
/* mmvae_dropout_advance(states[i], 0) for n distinct towers in ONE launch: forward call 0 of every tower of a training
 * step, issued before the towers fork onto their streams */
#define MMVAE_DROPOUT_ADVANCE_MAX 16
int mmvae_dropout_advance_many(uint32_t* const* states, int n, mmvae_stream_t stream);
/* out[i] = 0 or 1/(1-p): the multiplicative mask of element i (test / inspection helper) */
int mmvae_dropout_mask(const mmvae_dropout_t* drop, float* out, long n, mmvae_stream_t stream);
/* y = dropout(act(x)) elementwise; dx = dy * mask * act'(x).  act: MMVAE_ACT_NONE or MMVAE_ACT_GELU */
int mmvae_dropout_act_fwd(const float* x, float* y, long n, int act, const mmvae_dropout_t* drop,
                          mmvae_stream_t stream);
int mmvae_dropout_act_bwd(const float* dy, const float* x, float* dx, long n, int act, const mmvae_dropout_t* drop,
                          mmvae_stream_t stream);
/* cross-attention over a length-1 memory with attention-weight dropout (nn.MultiheadAttention dropout on the
 * (N*H, L, 1) weights): out[l,n,c] = v[n,c] * mask[(n*H + head(c))*L + l];  bwd: dv[n,c] = sum_l dout * mask */
int mmvae_head_bcast_dropout_fwd(const float* v, float* out, int L, int N, int H, int hd, const mmvae_dropout_t* drop,
                                 mmvae_stream_t stream);
int mmvae_head_bcast_dropout_bwd(const float* dout, float* dv, int L, int N, int H, int hd,
                                 const mmvae_dropout_t* drop, mmvae_stream_t stream);

/* Feed-forward block of nn.TransformerEncoderLayer / DecoderLayer with d_model = 32 (the action towers, reference
 * models/encoders.py:706-716, models/decoders.py:589-600) without materialising the (M, FF) hidden activation:
 *   y = W2 dropout(gelu(W1 x + b1)) + b2;   x, y (M,32); w1 (FF,32), b1 (FF), w2 (32,FF), b2 (32); FF % 32 == 0.
 * The dropout mask of hidden element (row, col) is that of mmvae_dropout_act_fwd at index row*FF + col (drop NULL or
 * p == 0: none).  Backward recomputes the hidden tiles: dx (M,32; may be NULL) and mmvae_ffn32_bwd_parts(M, FF) partial
 * rows of mmvae_ffn32_bwd_rowlen(FF) floats in ws, each [dW1 (FF,32) | db1 (FF) | dW2 (32,FF) | db2 (32)], to be summed
 * by the caller (mmvae_reduce_rows / mmvae_reduce_segments).  ws may be NULL too (data gradient only): the data- and
 * the weight-gradient launch are independent and may go to different streams. */
int mmvae_ffn32_supported(int d_model, int FF);
/* out_proj + dropout + residual + LayerNorm of a d_model-32 layer in one launch (reference models/encoders.py:706-716:
 * `src = norm1(src + dropout1(attn))`, the attention's out_proj being nn.Linear(32, 32)):
 *   y = LayerNorm(dropout(x W^T + b) + r);  x, r, y, xhat (M, 32), w (32, 32) [out][in], rstd (M); all 16-byte aligned.
 * Same saved tensors and dropout mask (element row * 32 + column) as mmvae_layernorm_residual_fwd on the Linear's output:
 * the backward is mmvae_layernorm_residual_bwd followed by the Linear's backward. */
int mmvae_proj32_ln_fwd(const float* x, const float* w, const float* b, const float* r, const float* gamma, const float* beta,
                        float* y, float* xhat, float* rstd, int M, const mmvae_dropout_t* drop, mmvae_stream_t stream);
int mmvae_ffn32_bwd_parts(int M, int FF);
size_t mmvae_ffn32_bwd_rowlen(int FF);
int mmvae_ffn32_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, int M,
                    int FF, const mmvae_dropout_t* drop, mmvae_stream_t stream);
int mmvae_ffn32_bwd(const float* x, const float* dy, const float* w1, const float* b1, const float* w2, float* dx,
                    float* ws, int M, int FF, const mmvae_dropout_t* drop, mmvae_stream_t stream);
/* The same three launches on split-bf16 MFMA (every fp32 operand = the exact sum of three bf16 terms, six bf16 MFMAs per
 * product, fp32 accumulation: the contract of the fp32 kernels above to ~3e-7 of the tensor maximum).  The weights are
 * split ONCE per step into wsplit (mmvae_ffn32_wsplit_bytes(FF) bytes, 16-byte aligned; mmvae_ffn32_prep_weights) and
 * that image replaces w1 / w2 in the calls; the weight-gradient launch also needs rsplit (mmvae_ffn32_rsplit_bytes(M)
 * bytes of scratch, written and read by that call in stream order).  Same partial-row layout in ws, same dropout mask.
 * dx_add (M,32) or NULL is added to dx (the gradient of the residual connection around the block). */
size_t mmvae_ffn32_wsplit_bytes(int FF);
size_t mmvae_ffn32_rsplit_bytes(int M);
int mmvae_ffn32_prep_weights(const float* w1, const float* w2, void* wsplit, int FF, mmvae_stream_t stream);
/* ... of up to 16 layers (host arrays of n device pointers each) in ONE launch */
int mmvae_ffn32_prep_weights_many(const float* const* w1, const float* const* w2, void* const* wsplit, int n, int FF,
                                  mmvae_stream_t stream);
int mmvae_ffn32_fwd_b16(const float* x, const void* wsplit, const float* b1, const float* b2, float* y, int M, int FF,
                        const mmvae_dropout_t* drop, mmvae_stream_t stream);
/* ... with the LayerNorm that consumes the block as the launch's epilogue: y = LayerNorm(dropout(ffn(x)) + r), xhat (M, 32)
 * and rstd (M) saved as mmvae_layernorm_residual_fwd saves them (ln_drop: the dropout in front of the residual sum, mask of
 * element row * 32 + column); backward = mmvae_layernorm_residual_bwd, then mmvae_ffn32_bwd_b16.
 * (reference models/encoders.py:706-716: `src = norm2(src + dropout2(linear2(dropout(activation(linear1(src))))))`) */
int mmvae_ffn32_fwd_b16_ln(const float* x, const void* wsplit, const float* b1, const float* b2, const float* r,
                           const float* gamma, const float* beta, float* y, float* xhat, float* rstd, int M, int FF,
                           const mmvae_dropout_t* drop, const mmvae_dropout_t* ln_drop, mmvae_stream_t stream);
int mmvae_ffn32_bwd_b16(const float* x, const float* dy, const void* wsplit, const float* b1, float* dx, float* ws,
                        void* rsplit, const float* dx_add, int M, int FF, const mmvae_dropout_t* drop,
                        mmvae_stream_t stream);

int mmvae_version(void);
const char* mmvae_arch(void); /* "gfx950" */

/* ------------------------------------------------------------------------------------------------
 * 4x4 / stride 2 / padding 1 convolutions, NCHW fp32, square maps  (a2, a3 of SURVEY 8(a))
 *   conv2d      : torch.nn.Conv2d(k=4,s=2,p=1)          models/encoders.py:186-191,214-217
 *   convT2d     : torch.nn.ConvTranspose2d(k=4,s=2,p=1)  models/decoders.py:62-69,91-95
 * Implicit GEMM on v_mfma_f32_32x32x2_f32 / 16x16x4_f32, im2col tiles staged through LDS.
 * Supported channel pairs: (3|32) -> 32 for the "gather" form, 32 -> (32|3) for the "scatter" form.
 * ---------------------------------------------------------------------------------------------- */

/* y[b,o,oh,ow] = ep( bias[o] + sum_{c,kh,kw} act(x[b,c,2oh-1+kh,2ow-1+kw]) * w[o,c,kh,kw] )
 * x (B,Cin,Hin,Hin) -> y (B,Cout,Hin/2,Hin/2); w (Cout,Cin,4,4).  bias/aux may be NULL. */
int mmvae_conv2d_k4s2_fwd(const float* x, const float* w, const float* bias, const float* aux, float* y,
                          int B, int Cin, int Cout, int Hin, int in_act, int ep_mode, mmvae_stream_t stream);

/* dx[b,c,ih,iw] = ep( sum_{o,kh,kw: ih=2oh-1+kh, iw=2ow-1+kw} dy[b,o,oh,ow] * w[o,c,kh,kw] )
 * dy (B,Cout,Hout,Hout) -> dx (B,Cin,2Hout,2Hout); w (Cout,Cin,4,4).  ep: MUL_* with aux = saved input. */
int mmvae_conv2d_k4s2_dgrad(const float* dy, const float* w, const float* aux, float* dx,
                            int B, int Cin, int Cout, int Hout, int ep_mode, mmvae_stream_t stream);

/* dw[o,c,kh,kw] (+)= sum_{b,oh,ow} dy[b,o,oh,ow] * act(x[b,c,2oh-1+kh,2ow-1+kw]);  db[o] (+)= sum dy.
 * ws: mmvae_conv_wgrad_ws_floats(B,Cin,Cout,Hout) floats. */
int mmvae_conv2d_k4s2_wgrad(const float* dy, const float* x, float* dw, float* db, float* ws,
                            int B, int Cin, int Cout, int Hout, int x_act, int accumulate, mmvae_stream_t stream);

/* y[b,o,oh,ow] = ep( bias[o] + sum_{c,kh,kw: oh=2ih-1+kh, ow=2iw-1+kw} act(x[b,c,ih,iw]) * w[c,o,kh,kw] )
 * x (B,Cin,Hin,Hin) -> y (B,Cout,2Hin,2Hin); w (Cin,Cout,4,4). */
int mmvae_convT2d_k4s2_fwd(const float* x, const float* w, const float* bias, const float* aux, float* y,
                           int B, int Cin, int Cout, int Hin, int in_act, int ep_mode, mmvae_stream_t stream);

/* dx[b,c,ih,iw] = ep( sum_{o,kh,kw} dy[b,o,2ih-1+kh,2iw-1+kw] * w[c,o,kh,kw] );  dy (B,Cout,2Hin,2Hin) */
int mmvae_convT2d_k4s2_dgrad(const float* dy, const float* w, const float* aux, float* dx,
                             int B, int Cin, int Cout, int Hin, int ep_mode, mmvae_stream_t stream);

/* dw[c,o,kh,kw] (+)= sum_{b,ih,iw} act(x[b,c,ih,iw]) * dy[b,o,2ih-1+kh,2iw-1+kw];  db[o] (+)= sum dy. */
int mmvae_convT2d_k4s2_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws,
                             int B, int Cin, int Cout, int Hin, int x_act, int accumulate, mmvae_stream_t stream);

size_t mmvae_conv_wgrad_ws_floats(int B, int Csmall, int Clarge, int Hsmall);

/* Whole-layer backward in ONE launch (input-gradient and weight-gradient workgroups side by side):
 *   conv2d : dx = dgrad(dy, w) * act'(x);  dw (+)= wgrad(dy, act(x));  db (+)= sum dy      x (B,Cin,2Hout,2Hout)
 *   convT2d: dx = dgrad(dy, w) * act'(x);  dw (+)= wgrad(act(x), dy);  db (+)= sum dy      dy (B,Cout,2Hin,2Hin)
 * ws as for the *_wgrad entry points; shapes that are not fused fall back to two launches. */
int mmvae_conv2d_k4s2_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, float* ws,
                          int B, int Cin, int Cout, int Hout, int x_act, int accumulate, mmvae_stream_t stream);
int mmvae_convT2d_k4s2_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, float* ws,
                           int B, int Cin, int Cout, int Hin, int x_act, int accumulate, mmvae_stream_t stream);
/* The weight-gradient halves of several mmvae_convT2d_k4s2_bwd launches in ONE launch of their own (their data
 * gradients: mmvae_convT2d_k4s2_dgrad): job j leaves in ws exactly the partial rows (mmvae_conv_wgrad_layout) that
 * mmvae_convT2d_k4s2_bwd(.., accumulate = MMVAE_ACC_DEFER) leaves for the same layer, for the caller's fold.  Serves the
 * two large layers of Dec_CNN (models/decoders.py:62-69): (Cin, Cout, Hin) = (32, 3, 32) and (32, 32, 16); any other
 * geometry, jobs whose splits call for different loop forms, or n_jobs > MMVAE_CONV_WGRAD_BATCH_MAX:
 * MMVAE_ERR_UNSUPPORTED. */
#define MMVAE_CONV_WGRAD_BATCH_MAX 4
typedef struct {
  const float* x; const float* dy; float* ws;      /* x (B,Cin,Hin,Hin), dy (B,Cout,2Hin,2Hin) */
  int B, Cin, Cout, Hin, x_act, has_bias;
} mmvae_conv_wgrad_job_t;
int mmvae_conv_wgrad_batch(const mmvae_conv_wgrad_job_t* jobs, int n_jobs, mmvae_stream_t stream);
/* Dec_CNN's last layer and its reconstruction loss in ONE launch (round 5; csrc/conv_t3.inc):
 *   logits = convT2d(act(x), w, bias)  x (B,32,32,32) -> (B,3,64,64)       models/decoders.py:69,95
 *   x_hat  = clamp(sigmoid(logits), 1e-6, 1 - 1e-6)                         models/decoders.py:96-97   (never stored)
 *   row[b] = sum bce(x_hat[b], target[b])   (logs clamped at -100)          models/objectives.py:392-406
 *   dlogit = seed * (x_hat - target) where the clamp is inactive, else 0    (the term's ELBO weight is known: ops.ConstSeed)
 * part: (B, mmvae_convT3_bce_strips(B)) floats and ticket: (B) unsigned, zeroed once by the caller (the kernel leaves the
 * tickets zero), when an image is split over several workgroups (strips > 1); both may be NULL when strips == 1. */
int mmvae_convT3_bce_seeded(const float* x, const float* w, const float* bias, const float* target, float* row,
                            float* dlogit, float* part, unsigned* ticket, int B, int in_act, float seed,
                            mmvae_stream_t stream);
int mmvae_convT3_bce_strips(int B);
/* The 32-channel layers on 16x16 / 32x32 maps and the 3-channel image layers run on one of two GEMM cores from a
 * tile-count threshold on: "split-bf16" (every fp32 operand split EXACTLY into three bf16 terms, six bf16 MFMAs per
 * product, fp32 accumulate; dropped terms <= 3 * 2^-24 |a b|, i.e. fp32-equivalent: tests/test_hip_ops.py holds it to
 * 2e-6 of the tensor maximum against fp64) or fp32 MFMA.  split_bf16 = 1 (default) / 0 selects, < 0 keeps; returns the
 * previous setting.  Non-finite inputs: see DESIGN.md "split-bf16 and non-finite values". */
int mmvae_conv_plan(int split_bf16);

/* ------------------------------------------------------------------------------------------------
 * Small dense layers: torch.nn.Linear and the projections inside nn.MultiheadAttention /
 * nn.Transformer*Layer  (models/encoders.py:194,43-54,825-826; models/decoders.py:58-60,86-88,705)
 * One strided fp32 MFMA GEMM:  C[M,N] = ep( bias + act(A)[M,K] * B[K,N] )
 *   A(m,k) at A[m*sam + k*sak],  B(k,n) at Bm[k*sbk + n*sbn],  C row-major with leading dim ldc.
 *   bias: per column n, or NULL.  a_rowsum (optional, length M): (+)= sum_k act(A)(m,k)
 *   (the bias gradient when A = dy^T).  splitk > 1 needs ws of mmvae_gemm_ws_floats() floats and
 *   allows neither bias nor epilogue (partials are summed by mmvae_reduce_rows: unless deferred, ldc must be N then,
 *   or MMVAE_ERR_UNSUPPORTED).
 * ---------------------------------------------------------------------------------------------- */
int mmvae_gemm_f32(const float* A, const float* Bm, const float* bias, const float* aux, float* C,
                   float* a_rowsum, float* ws, int M, int N, int K, long sam, long sak, long sbk, long sbn,
                   long ldc, int a_act, int b_act, int ep_mode, int accumulate, int splitk,
                   mmvae_stream_t stream);
size_t mmvae_gemm_ws_floats(int M, int N, int splitk);
/* number of partial results (rows of M*N [+ M] floats in ws) mmvae_gemm_f32 writes for a requested splitk */
int mmvae_gemm_splits(int M, int N, int K, int splitk);
/* Runtime switch of the LDS-tiled split-bf16 kernels that take wide layers (N, K >= 128) at 2048 .. 4096 rows over from the
 * fp32-MFMA bodies in mmvae_gemm_f32 / mmvae_linear_fwd / _bwd_data / _bwd (csrc/gemm_b16.inc; same fp32 contract, every
 * product from six bf16 MFMAs on three exact bf16 terms per operand).  Returns the previous setting; the environment
 * variable MMVAE_GEMM_B16=0 starts with it off.  (nn.Linear: reference models/encoders.py:196-200, models/decoders.py:58-62.) */
int mmvae_gemm_b16_set(int on);
/* grouped bias of a layer whose N outputs are C channels x G positions (nn.ConvTranspose2d on a 1x1 input run as a
 * GEMM, models/decoders.py:116,129-131):  y[r, c*G + g] += bias[c];   db[c] (+)= sum_r sum_g dy[r, c*G + g] */
int mmvae_bias_group_add(float* y, const float* bias, int rows, int C, int G, mmvae_stream_t stream);
size_t mmvae_bias_group_ws_floats(int rows, int C);   /* = parts * C; parts = mmvae_bias_group_parts(rows) */
int mmvae_bias_group_parts(int rows);
/* ws: mmvae_bias_group_ws_floats floats of row-block partials (parts, C); accumulate = MMVAE_ACC_DEFER leaves them
 * there for the caller's fold */
int mmvae_bias_group_grad(const float* dy, float* db, float* ws, int rows, int C, int G, int accumulate,
                          mmvae_stream_t stream);

/* y = ep(x W^T + b): x (M,K) ld ldx, W (N,K), y (M,N).  F.linear */
int mmvae_linear_fwd(const float* x, const float* w, const float* b, float* aux, float* y, int M, int N, int K,
                     long ldx, int x_act, int ep_mode, mmvae_stream_t stream);
/* dx = ep(dy W): dy (M,N), W (N,K), dx (M,K) */
int mmvae_linear_bwd_data(const float* dy, const float* w, const float* aux, float* dx, int M, int N, int K,
                          int ep_mode, int accumulate, mmvae_stream_t stream);
/* dW (+)= dy^T act(x), db (+)= colsum(dy); dW (N,K).  ws: mmvae_linear_bwd_weight_ws_floats(M,N,K) */
int mmvae_linear_bwd_weight(const float* dy, const float* x, float* dw, float* db, float* ws, int M, int N, int K,
                            long ldx, int x_act, int accumulate, mmvae_stream_t stream);
size_t mmvae_linear_bwd_weight_ws_floats(int M, int N, int K);
/* Several independent weight gradients (the (L*N)-row ones a fused text layer leaves behind) in ONE launch: every
 * job gets exactly the tiling / split plan / partial layout of mmvae_linear_bwd_weight, so results are bit-identical to
 * n_jobs separate calls -- which is also what happens when a job falls outside the shared-grid regime (the
 * register-operand body; split jobs need accumulate == MMVAE_ACC_DEFER) or n_jobs > MMVAE_WGRAD_BATCH_MAX.
 * Replaces the autograd-generated per-Linear weight-gradient matmuls of nn.TransformerEncoderLayer /
 * nn.TransformerDecoderLayer.backward (reference models/encoders.py:818-824, models/decoders.py:698-704). */
#define MMVAE_WGRAD_BATCH_MAX 8
typedef struct {
  const float* dy; const float* x; float* dw; float* db; float* ws;
  int M, N, K; long ldx; int x_act, accumulate;
} mmvae_wgrad_job_t;
int mmvae_linear_bwd_weight_batch(const mmvae_wgrad_job_t* jobs, int n_jobs, mmvae_stream_t stream);
/* All weight gradients behind one fused text layer in ONE launch (csrc/twgrad.hip; round 4): dW_j = dy_j^T x_j and
 * db_j = colsum(dy_j) of torch.nn.TransformerEncoderLayer / TransformerDecoderLayer's linears
 * (models/encoders.py:828-837, models/decoders.py:708-723), each operand row fetched once.  Every job writes
 * nz = mmvae_txt_wgrad_splits(M, N, K) partial rows to ws, row z at ws + z * pitch = [N * K weight sums | N bias sums]
 * with pitch = mmvae_txt_wgrad_ws_floats(M, N, K) / nz (N * K + N rounded up to even), to be folded by
 * mmvae_reduce_segments / mmvae_adam_fold_flat -- as ONE segment of length N * K + N when weight and bias are adjacent in
 * the gradient buffer.  N (K) must be even when > 32. */
typedef struct {
  const float* dy; const float* x; float* ws;
  int M, N, K;
} mmvae_txt_wgrad_job_t;
int mmvae_txt_wgrad(const mmvae_txt_wgrad_job_t* jobs, int n_jobs, mmvae_stream_t stream);
int mmvae_txt_wgrad_splits(int M, int N, int K);
size_t mmvae_txt_wgrad_ws_floats(int M, int N, int K);
int mmvae_txt_wgrad_supported(int M, int N, int K);
/* both of the above in one grouped launch: dx = ep(dy W), dW (+)= dy^T act(x), db (+)= colsum(dy) */
int mmvae_linear_bwd(const float* dy, const float* x, const float* w, const float* aux, float* dx, float* dw,
                     float* db, float* ws, int M, int N, int K, long ldx, int x_act, int ep_mode, int accumulate,
                     mmvae_stream_t stream);
size_t mmvae_linear_bwd_ws_floats(int M, int N, int K);

/* Which kernel instantiation of csrc/gemm.hip serves a call: one value per instantiation, returned by the three queries
 * below and switched on by mmvae_gemm_f32 / mmvae_linear_fwd / mmvae_linear_bwd themselves (the query IS the dispatch).
 * Operand orientation suffix: A then B, K = reduction index contiguous in memory, M / N = row / column index contiguous.
 * Load suffix of the register-operand kernels: A then B, V = float4 along k, S = strided dwords.
 *   B16_<o>_<g>       gemm_b16_kernel (split-bf16 LDS tiles), g k-groups per tile
 *   BIG<bn>_<o>       gemm_big_kernel, 128 x bn tiles
 *   RSPLIT_<d>        rgemm_kernel<d, false, false> with gridDim.z = nz > 1 (weight gradients with few tiles)
 *   R16_<d>_<l>       rgemm16_kernel (16 x 16 tiles), reduction slices d deep
 *   R32_<d>_<l>       rgemm_kernel (32 x 32 tiles), one split
 *   STAGED<v>_<o>     gemm_kernel<v, ..> (LDS staged; v = 1: 128 x 32 tiles, 4 / 8: 32 x 32 tiles over 4 / 8 waves)
 *   PROJ32            the 32-wide projection of csrc/ffn.hip (mmvae_linear_fwd only)
 *   LINBWD_B16_<g>    gemm_b16_linear_bwd_kernel<g>
 *   LINBWD_R_<d>_T<t> rgemm_grouped_kernel<d, 16, t == 16>: data gradient d deep on t x t tiles
 *   LINBWD_STAGED     gemm_grouped_kernel
 *   LINBWD_TWO        mmvae_linear_bwd_weight, then mmvae_linear_bwd_data (each with its own path) */
enum {
  MMVAE_GEMM_B16_KK_1 = 16,
  MMVAE_GEMM_B16_KN_1,
  MMVAE_GEMM_B16_MK_1,
  MMVAE_GEMM_B16_MN_1,
  MMVAE_GEMM_B16_KK_2,
  MMVAE_GEMM_B16_KN_2,
  MMVAE_GEMM_B16_MK_2,
  MMVAE_GEMM_B16_MN_2,
  MMVAE_GEMM_BIG128_KK,
  MMVAE_GEMM_BIG128_KN,
  MMVAE_GEMM_BIG128_MK,
  MMVAE_GEMM_BIG128_MN,
  MMVAE_GEMM_BIG64_KK,
  MMVAE_GEMM_BIG64_KN,
  MMVAE_GEMM_BIG64_MK,
  MMVAE_GEMM_BIG64_MN,
  MMVAE_GEMM_RSPLIT_16,
  MMVAE_GEMM_RSPLIT_64,
  MMVAE_GEMM_R16_16_VV,
  MMVAE_GEMM_R16_16_VS,
  MMVAE_GEMM_R16_16_SV,
  MMVAE_GEMM_R16_16_SS,
  MMVAE_GEMM_R16_64_VV,
  MMVAE_GEMM_R16_64_VS,
  MMVAE_GEMM_R16_64_SV,
  MMVAE_GEMM_R16_64_SS,
  MMVAE_GEMM_R32_16_VV,
  MMVAE_GEMM_R32_16_VS,
  MMVAE_GEMM_R32_16_SV,
  MMVAE_GEMM_R32_16_SS,
  MMVAE_GEMM_R32_64_VV,
  MMVAE_GEMM_R32_64_VS,
  MMVAE_GEMM_R32_64_SV,
  MMVAE_GEMM_R32_64_SS,
  MMVAE_GEMM_STAGED1_KK,
  MMVAE_GEMM_STAGED1_KN,
  MMVAE_GEMM_STAGED1_MK,
  MMVAE_GEMM_STAGED1_MN,
  MMVAE_GEMM_STAGED4_KK,
  MMVAE_GEMM_STAGED4_KN,
  MMVAE_GEMM_STAGED4_MK,
  MMVAE_GEMM_STAGED4_MN,
  MMVAE_GEMM_STAGED8_KK,
  MMVAE_GEMM_STAGED8_KN,
  MMVAE_GEMM_STAGED8_MK,
  MMVAE_GEMM_STAGED8_MN,
  MMVAE_GEMM_PROJ32,
  MMVAE_GEMM_LINBWD_B16_1,
  MMVAE_GEMM_LINBWD_B16_2,
  MMVAE_GEMM_LINBWD_R_16_T32,
  MMVAE_GEMM_LINBWD_R_16_T16,
  MMVAE_GEMM_LINBWD_R_64_T32,
  MMVAE_GEMM_LINBWD_R_64_T16,
  MMVAE_GEMM_LINBWD_STAGED,
  MMVAE_GEMM_LINBWD_TWO
};
/* THE dispatch rule of mmvae_gemm_f32, as a pure host query (no launch, no GPU needed): one of the values above, or a
 * NEGATED error: -MMVAE_ERR_ARG for a non-positive size, -MMVAE_ERR_UNSUPPORTED for strides no kernel takes (neither sak
 * nor sam is 1, or B is neither k-major nor sbn == 1).  has_rowsum: a_rowsum != NULL; a_al16 / b_al16: the operand pointer
 * is 16-byte aligned.  ldc and accumulate decide one thing: splits that the call sums itself (nz > 1, accumulate !=
 * MMVAE_ACC_DEFER) are written by mmvae_reduce_rows as M * N contiguous floats, so they need ldc == N, else
 * -MMVAE_ERR_UNSUPPORTED (deferred partials never touch C: any ldc).  nz_out / kper_out (may be NULL):
 * the number of reduction splits that write partials (1: straight to C) and the reduction length of one split. */
int mmvae_gemm_path(int M, int N, int K, long sam, long sak, long sbk, long sbn, long ldc, int a_act, int b_act,
                    int ep_mode, int accumulate, int splitk, int has_rowsum, int a_al16, int b_al16, int* nz_out,
                    int* kper_out);
/* ... of mmvae_linear_fwd: MMVAE_GEMM_PROJ32 or the mmvae_gemm_f32 path of (x, W).  out_al16: y and b 16-byte aligned */
int mmvae_linear_fwd_path(int M, int N, int K, long ldx, int x_act, int ep_mode, int x_al16, int w_al16, int out_al16);
/* ... of mmvae_linear_bwd_weight: the mmvae_gemm_f32 path of the (N x K) = dy^T act(x) problem with reduction length M and
 * the split request the wrapper makes.  has_db: db != NULL (the row sums of dy^T) */
int mmvae_linear_bwd_weight_path(int M, int N, int K, long ldx, int x_act, int accumulate, int has_db, int dy_al16,
                                 int x_al16, int* nz_out, int* kper_out);
/* ... of mmvae_linear_bwd: a MMVAE_GEMM_LINBWD_* value, or -MMVAE_ERR_ARG where the chosen grouped kernel needs an
 * alignment the call lacks (split-bf16: dy, x, W 16-byte aligned and ldx % 4 == 0; register-operand: dy).  nz_out: the
 * number of weight-gradient partials (= mmvae_linear_bwd_splits); kper_out: rows of the reduction per partial. */
int mmvae_linear_bwd_path(int M, int N, int K, long ldx, int x_act, int ep_mode, int accumulate, int has_db, int dy_al16,
                          int x_al16, int w_al16, int* nz_out, int* kper_out);

/* ------------------------------------------------------------------------------------------------
 * Encoder heads: VaeComponent.process_output, models/encoders.py:49-54
 *   h (B, 2D) = [mu | pre-softmax]  ->  lv = softmax(h[:, D:], -1) + 1e-6, written in place.
 * bwd: dh[:, D:] = softmax backward of dlv (in place on dh, which holds [dmu | dlv]).
 * ---------------------------------------------------------------------------------------------- */
int mmvae_head_softmax_fwd(float* h, int B, int D, mmvae_stream_t stream);
int mmvae_head_softmax_bwd(const float* h, float* dh, int B, int D, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused latent op: product of experts -> reparameterised samples -> analytic KL
 *   TorchMMVAE.product_of_experts   models/mmvae_base.py:203-222   (returns VARIANCE, used as sigma)
 *   MoPOE.poe_fusion / forward      models/mmvae_models.py:385-394,351-370
 *   POE.modality_mixing / forward   models/mmvae_models.py:189-232
 *   weighted_group_kld / kl_normal  models/objectives.py:184-201, utils.py:399-402
 *   model prior sigma = softmax(theta)*D  models/mmvae_models.py:274-276
 *
 * experts: E pointers (device array of E device pointers is NOT used; pass up to 8 pointers by value)
 *   mu[e], lv[e] : (B,D) each with row stride ld_in (2D when they are the halves of a packed head output;
 *                  dmu/dlv use the same stride); lv is the encoder's softmax output, used as log-variance
 *                  inside PoE.  eps, z, dz are contiguous (B,D).
 *   with_prior   : 0 = product of the experts only; 1 = add the N(0,1) expert (mu 0, logvar 0);
 *                  2 = no product (E must be 1): the "joint" is expert 0 itself with sigma = its lv -- the
 *                  per-modality posteriors of MoE (models/mmvae_models.py:96-100).  Not with raw_heads
 *                  (MMVAE_ERR_ARG, both directions): lv_0 is the scale as it stands.
 *   n_z draws    : z[i] = mu_J + var_J * eps[i]   (eps[i], z[i] : (B,D))
 *   kl (n_kl,B)  : row j < E: sum_d KL(N(mu_j, sigma=lv_j) || p) if kl_mask bit j set;
 *                  row E    : sum_d KL(N(mu_J, sigma=var_J) || p) if kl_mask bit E set; p = N(0, softmax(theta)*D)
 *   joint (2,B,D): mu_J, var_J (always written).
 * bwd: dz[i] (B,D), dkl (E+1,B)  ->  dmu[e], dlv[e] (B,D), dtheta (D) (+)=; ws: mmvae_poe_ws_floats(B,D).
 *   raw_heads    : != 0: lv[e] points at the RAW logvar-head outputs u and the kernels apply
 *                  lv = softmax(u, -1) + 1e-6 themselves (process_output, encoders.py:52-53), forward and backward
 *                  (dlv[e] then receives d/du) -- no mmvae_head_softmax_* launch per tower and direction.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_MAX_EXPERTS 8
typedef struct {
  const float* mu[MMVAE_MAX_EXPERTS];
  const float* lv[MMVAE_MAX_EXPERTS];
  const float* eps[MMVAE_MAX_EXPERTS];
  float* z[MMVAE_MAX_EXPERTS];
} mmvae_poe_fwd_args;
typedef struct {
  const float* mu[MMVAE_MAX_EXPERTS];
  const float* lv[MMVAE_MAX_EXPERTS];
  const float* eps[MMVAE_MAX_EXPERTS];
  const float* dz[MMVAE_MAX_EXPERTS];
  float* dmu[MMVAE_MAX_EXPERTS];
  float* dlv[MMVAE_MAX_EXPERTS];
} mmvae_poe_bwd_args;
/* rng_state: NULL (a->eps are inputs), or the mmvae_randn generator state: the n_z draws are then generated by this
 * launch -- element i*B*D + b*D + d of the current draw, the values mmvae_randn would put into a (n_z,B,D) tensor --
 * written to a->eps[i] (outputs, kept for the backward pass), and the generator advances by one draw */
int mmvae_poe_reparam_kl_fwd(const mmvae_poe_fwd_args* a, const float* theta, float* joint, float* kl, int E,
                             int with_prior, int n_z, unsigned kl_mask, int B, int D, int ld_in, int raw_heads,
                             uint32_t* rng_state, mmvae_stream_t stream);
/* ticket: NULL, or a zero-initialised device int owned by the calling stream: the prior-parameter gradient is then
 * folded by the last workgroup of the same launch (the kernel leaves the int at zero) instead of a second launch */
int mmvae_poe_reparam_kl_bwd(const mmvae_poe_bwd_args* a, const float* theta, const float* dkl, float* dtheta,
                             float* ws, int* ticket, int E, int with_prior, int n_z, unsigned kl_mask, int B, int D,
                             int ld_in, int raw_heads, int accumulate, mmvae_stream_t stream);
/* ... acc_packed bit e: dmu[e] / dlv[e] already hold another call's contribution to these columns and this one is ADDED (the
 * same head output read by several fusion calls -- DMVAE's joint, shared and private posteriors, models/mmvae_models.py:
 * 480-502 -- accumulates its gradient in one tensor instead of one tensor per call plus autograd's addition launches).
 * Not with raw_heads. */
int mmvae_poe_reparam_kl_bwd_acc(const mmvae_poe_bwd_args* a, const float* theta, const float* dkl, float* dtheta,
                                 float* ws, int* ticket, int E, int with_prior, int n_z, unsigned kl_mask, int B, int D,
                                 int ld_in, int raw_heads, int accumulate, unsigned acc_packed, mmvae_stream_t stream);
size_t mmvae_poe_ws_floats(int B, int D);

/* ------------------------------------------------------------------------------------------------
 * Total-correlation fusion (MVTCAE: Hwang et al., NeurIPS 2021): product of experts -> ONE reparameterised sample ->
 * KL of the joint to the prior AND KL of the joint to every expert, forward and backward (csrc/tcfusion.hip).
 * The conventions are those of mmvae_poe_reparam_kl_*: up to MMVAE_MAX_EXPERTS expert pointers by value, mu[e] / lv[e]
 * (and dmu[e] / dlv[e]) with row stride ld_in, eps / z / dz contiguous (B,D), raw_heads != 0: lv[e] points at the raw
 * logvar-head output u and lv = softmax(u, -1) + 1e-6 is applied here, forward and backward (dlv[e] receives d/du; one
 * column: du = 0).  The product's variance is used as the scale, as everywhere in this library.
 *   T_e = 1 / (exp(lv_e) + 1e-8), P = sum_e T_e, mu_J = sum_e mu_e T_e / P, V_J = 1 / P (no prior expert),
 *   z = mu_J + V_J eps, sp = softmax(theta) D
 *   joint (2,B,D) : mu_J, V_J
 *   kl (E+1,B)    : row E: sum_d KL(N(mu_J, sigma = V_J) || N(0, sp))
 *                   row e: sum_d KL(N(mu_J, sigma = V_J) || N(mu_e, sigma = 1 / T_e))
 *                          = sum_d [ -log(T_e V_J) + T_e^2 (V_J^2 + (mu_J - mu_e)^2) / 2 - 1 / 2 ]
 * bwd: dz (B,D), dkl (E+1,B) -> dmu[e], dlv[e], dtheta (D) (accumulate != 0: added to what dtheta holds).  dz / dkl NULL: an
 *   absent upstream gradient, taken as zeros; dtheta NULL: the prior gradient is not wanted (no second launch).  Nothing is
 *   detached: row e differentiates through the joint and through expert e's own parameters.  Every workgroup writes its
 *   partial prior-gradient row to ws (mmvae_tc_fusion_ws_floats(B, D) floats), a second one-workgroup launch folds them:
 *   every sum in one fixed order, no atomics -- the results are bit-reproducible from run to run.
 * 1 <= E <= MMVAE_MAX_EXPERTS and D <= 256; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing
 * (mmvae_tc_fusion_ws_floats: 0).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* mu[MMVAE_MAX_EXPERTS];
  const float* lv[MMVAE_MAX_EXPERTS];
} mmvae_tc_fwd_args;
typedef struct {
  const float* mu[MMVAE_MAX_EXPERTS];
  const float* lv[MMVAE_MAX_EXPERTS];
  float* dmu[MMVAE_MAX_EXPERTS];
  float* dlv[MMVAE_MAX_EXPERTS];
} mmvae_tc_bwd_args;
int mmvae_tc_fusion_fwd(const mmvae_tc_fwd_args* a, const float* theta, const float* eps, float* joint, float* kl,
                        float* z, int E, int B, int D, int ld_in, int raw_heads, mmvae_stream_t stream);
int mmvae_tc_fusion_bwd(const mmvae_tc_bwd_args* a, const float* theta, const float* eps, const float* dz,
                        const float* dkl, float* dtheta, float* ws, int E, int B, int D, int ld_in, int raw_heads,
                        int accumulate, mmvae_stream_t stream);
size_t mmvae_tc_fusion_ws_floats(int B, int D);

/* ------------------------------------------------------------------------------------------------
 * Jensen-Shannon fusion (mmJSD: Sutter, Daunhawer, Vogt, NeurIPS 2020): the weighted geometric mean of the E unimodal
 * posteriors and the prior (the "dynamic prior"), the KL of each of the E + 1 to it, and ONE reparameterised sample per
 * row from the expert sel[b] names, forward and backward (csrc/jsfusion.hip).  Pointer tables, ld_in, raw_heads, eps / z /
 * dz, ws, dtheta and accumulate are those of mmvae_tc_fusion_*.  Expert j < E is N(mu_j, sigma_j = lv_j): the head is read
 * as the SCALE, as the mixture of experts samples from it; j = E is the prior N(0, sp), sp = softmax(theta) D.
 * weights: E + 1 host floats pi_0 .. pi_E (pi_E: the prior's), each finite and >= 0, their sum > 0, or MMVAE_ERR_ARG.
 *   T_j = pi_j / sigma_j^2, P = sum_j T_j, f = sum_j T_j mu_j / P, m_j = mu_j - f (formed from pairwise differences)
 *   prior (2,B,D) : f, P^-1/2                                  (not differentiable)
 *   kl (E+1,B)    : row j: sum_d KL(N(mu_j, sigma_j) || N(f, P^-1/2))
 *                          = sum_d [ -log(sigma_j^2 P) + P (sigma_j^2 + m_j^2) - 1 ] / 2            (unweighted)
 *   z (B,D)       : mu_s + sigma_s eps, s = sel[b] (int32, B values).  The expert is found by comparing indices: a value
 *                   outside [0, E) selects nothing, its z row is 0 and no gradient flows from it.
 * bwd: dz (B,D), dkl (E+1,B) -> dmu[e], dlv[e] (d/d sigma_e; raw_heads: d/du), dtheta as mmvae_tc_fusion_bwd; every sum in
 *   one fixed order, no atomics: bit-reproducible from run to run.
 * 1 <= E <= MMVAE_MAX_EXPERTS and D <= 256; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing
 * (mmvae_js_fusion_ws_floats: 0).
 * ---------------------------------------------------------------------------------------------- */
int mmvae_js_fusion_fwd(const mmvae_tc_fwd_args* a, const float* weights, const float* theta, const float* eps,
                        const int* sel, float* prior, float* kl, float* z, int E, int B, int D, int ld_in, int raw_heads,
                        mmvae_stream_t stream);
int mmvae_js_fusion_bwd(const mmvae_tc_bwd_args* a, const float* weights, const float* theta, const float* eps,
                        const int* sel, const float* dz, const float* dkl, float* dtheta, float* ws, int E, int B, int D,
                        int ld_in, int raw_heads, int accumulate, mmvae_stream_t stream);
size_t mmvae_js_fusion_ws_floats(int B, int D);

/* ------------------------------------------------------------------------------------------------
 * Mixture-of-experts prior (MMVM VAE: Sutter et al., "Unity by Diversity", NeurIPS 2024): ONE reparameterised sample from
 * EVERY one of the E unimodal posteriors, the one-sample estimate of each posterior's KL to the uniform mixture of all E
 * (the data-dependent prior), its closed-form KL to the fixed prior and the responsibilities, forward and backward
 * (csrc/mixprior.hip).  The pointer tables are those of mmvae_poe_reparam_kl_*: mu[e] / lv[e] rows are ld_in floats apart,
 * eps[e] / z[e] / dz[e] are contiguous (B,D); raw_heads, ws, dtheta and accumulate are those of mmvae_tc_fusion_*.  Expert j
 * is q_j = N(mu_j, sigma_j = lv_j): the head is read as the SCALE, as the mixture of experts samples from it; the fixed
 * prior is N(0, sp), sp = softmax(theta) D.  With z_m = mu_m + sigma_m eps_m:
 *   u_mj = ((mu_m - mu_j) + sigma_m eps_m) / sigma_j
 *   D_mj = sum_d [ -(u_mj - eps_m)(u_mj + eps_m) / 2 - log(sigma_j / sigma_m) ]  = log q_j(z_m) - log q_m(z_m), D_mm = 0
 *   z[m] (B,D)    : z_m
 *   kl (2E,B)     : row m     : log q_m(z_m) - log (1/E) sum_j q_j(z_m) = log E - log sum_j exp(D_mj)
 *                   row E + m : sum_d KL(N(mu_m, sigma_m) || N(0, sp))
 *   resp (E,E,B)  : resp[m][j] = softmax_j D_mj: the weight of q_j in the mixture density at z_m   (not differentiable)
 * The absolute log-densities are never formed.
 * bwd: dz[m] (B,D), dkl (2E,B), resp as the forward pass wrote it (the row sums are not taken again) -> dmu[e], dlv[e]
 *   (d/d sigma_e; raw_heads: d/du), dtheta as mmvae_tc_fusion_bwd.  dkl NULL and every dz[m] NULL on its own: an absent
 *   upstream gradient, taken as zeros.  Every sum in one fixed order, no atomics: bit-reproducible from run to run.
 * 1 <= E <= MMVAE_MAX_EXPERTS and D <= 256; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing
 * (mmvae_mixprior_ws_floats: 0).
 * ---------------------------------------------------------------------------------------------- */
int mmvae_mixprior_fwd(const mmvae_poe_fwd_args* a, const float* theta, float* kl, float* resp, int E, int B, int D,
                       int ld_in, int raw_heads, mmvae_stream_t stream);
int mmvae_mixprior_bwd(const mmvae_poe_bwd_args* a, const float* theta, const float* resp, const float* dkl,
                       float* dtheta, float* ws, int E, int B, int D, int ld_in, int raw_heads, int accumulate,
                       mmvae_stream_t stream);
size_t mmvae_mixprior_ws_floats(int B, int D);

/* ------------------------------------------------------------------------------------------------
 * MMVAE+ latent op, K = 1 (Palumbo, Daunhawer, Vogt, ICLR 2023): shared and private latents of E modalities in one launch
 * each way (csrc/mmplus.hip).  Head e holds W = D + P columns per half: mu[e] / lv[e] point at (B, W) blocks whose rows are
 * ld_in floats apart (packed heads [mu | lv]: ld_in = 2 W); columns [0, D) are the SHARED posterior q_e^u, [D, W) the
 * PRIVATE one q_e^w, both N(mu, sigma = lv): the head is read as the SCALE.  raw_heads: lv = softmax(u, -1) + 1e-6 over
 * all W columns, applied here both ways (dlv[e] receives d/du; the softmax couples shared and private columns).  Priors:
 * p(u) = N(0, sp), sp = softmax(theta) D over the D shared columns; p(w) = N(0, 1).  eps_u (E,B,D), eps_w (E,B,P) and
 * eps_a (E,E,B,P), indexed [decoder n][source m] (the diagonal is never read; E = 1: may be NULL), are standard-normal
 * draws; aux_scale = s is the scale of the auxiliary cross prior r(w) = N(0, s^2): finite and > 0, or MMVAE_ERR_ARG.
 * With u_m = mu_m^u + sigma_m^u eps_u[m], w_m = mu_m^w + sigma_m^w eps_w[m]:
 *   z[n] (E B, W) : decoder n's whole input batch: row m B + b = [u_m[b] | w_m[b]] if n == m, else [u_m[b] | s eps_a[n][m][b]]
 *   kl (3E,B)     : row m      : log q_m^u(u_m) - log (1/E) sum_j q_j^u(u_m), in mmvae_mixprior_fwd's difference arithmetic
 *                   row E + m  : sum_d KL(q_m^u || N(0, sp))
 *                   row 2E + m : sum_p KL(q_m^w || N(0, 1))
 *   resp (E,E,B)  : resp[m][j] = the weight of q_j^u in the mixture density at u_m           (not differentiable)
 * bwd: dz[n] (E B, W) each, dkl (3E,B), resp as the forward pass wrote it -> dmu[e], dlv[e] over all W columns, dtheta (D)
 *   as mmvae_tc_fusion_bwd (ws: mmvae_mmplus_ws_floats(B, D, P) floats, accumulate, dtheta NULL).  The gradient of u_m is
 *   the sum over n = 0 .. E-1 of columns [0, D) of row block m of dz[n]; that of w_m is columns [D, W) of row block m of
 *   dz[m] alone.  dkl NULL and every dz[n] NULL on its own: an absent upstream gradient, taken as zeros.  Nothing is
 *   detached.  Every sum in one fixed order, no atomics: bit-reproducible from run to run.
 * 1 <= E <= MMVAE_MAX_EXPERTS, D >= 1, P >= 1 and D + P <= 256; anything else returns MMVAE_ERR_UNSUPPORTED and writes
 * nothing (mmvae_mmplus_ws_floats: 0).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* mu[MMVAE_MAX_EXPERTS];
  const float* lv[MMVAE_MAX_EXPERTS];
  float* z[MMVAE_MAX_EXPERTS];
} mmvae_mmplus_fwd_args;
typedef struct {
  const float* mu[MMVAE_MAX_EXPERTS];
  const float* lv[MMVAE_MAX_EXPERTS];
  const float* dz[MMVAE_MAX_EXPERTS];
  float* dmu[MMVAE_MAX_EXPERTS];
  float* dlv[MMVAE_MAX_EXPERTS];
} mmvae_mmplus_bwd_args;
int mmvae_mmplus_fwd(const mmvae_mmplus_fwd_args* a, const float* theta, const float* eps_u, const float* eps_w,
                     const float* eps_a, float aux_scale, float* kl, float* resp, int E, int B, int D, int P, int ld_in,
                     int raw_heads, mmvae_stream_t stream);
int mmvae_mmplus_bwd(const mmvae_mmplus_bwd_args* a, const float* theta, const float* eps_u, const float* eps_w,
                     const float* resp, const float* dkl, float* dtheta, float* ws, int E, int B, int D, int P, int ld_in,
                     int raw_heads, int accumulate, mmvae_stream_t stream);
size_t mmvae_mmplus_ws_floats(int B, int D, int P);

/* Latent samples -> decoder inputs, and the transpose (round 6).  The reference decodes every subset's sample in a call of its
 * own (POE.objective, models/mmvae_models.py:159-187) and builds DMVAE's decoder inputs with torch.cat([z_shared, z_private], -1)
 * per pass (:494-502); here a decoder's passes are one batch, and the batches of ALL decoders are written by one launch:
 * block k copies B rows of `width[k]` floats, dst[k][b * ld_dst[k] + d] = src[k][b * ld_src[k] + d] (dst already points at the
 * block's first row / column of its output).  bwd: out[s] (B, width[s]) = sum_j g[s][j][b * ld[s][j] + d] over the n_g[s] <= 4
 * blocks that read source s, in that order. */
#define MMVAE_FAN_MAX_BLOCKS 16
#define MMVAE_FAN_MAX_SRC 8
#define MMVAE_FAN_MAX_USES 4
typedef struct {
  const float* src[MMVAE_FAN_MAX_BLOCKS];
  float* dst[MMVAE_FAN_MAX_BLOCKS];
  int width[MMVAE_FAN_MAX_BLOCKS], ld_src[MMVAE_FAN_MAX_BLOCKS], ld_dst[MMVAE_FAN_MAX_BLOCKS];
  int n, B;
} mmvae_fan_blocks_t;
typedef struct {
  float* out[MMVAE_FAN_MAX_SRC];
  const float* g[MMVAE_FAN_MAX_SRC][MMVAE_FAN_MAX_USES];
  int ld[MMVAE_FAN_MAX_SRC][MMVAE_FAN_MAX_USES];
  int n_g[MMVAE_FAN_MAX_SRC], width[MMVAE_FAN_MAX_SRC];
  int n, B;
} mmvae_fan_sum_t;
int mmvae_rows_fan_fwd(const mmvae_fan_blocks_t* blocks, mmvae_stream_t stream);
int mmvae_rows_fan_bwd(const mmvae_fan_sum_t* sums, mmvae_stream_t stream);

/* MoE importance weights, models/mmvae_models.py:56-62:  lw[b] = sum_d [log N(z; mu_r, s_r) - log N(z; mu_o, s_o)]
 * with z and the source posterior detached; packed_* = (B,2D) [mu | sigma].  bwd: dpacked_r (B,2D) = g[b] * d lw. */
int mmvae_normal_logratio_fwd(const float* packed_r, const float* packed_o, const float* z, float* lw, int B, int D,
                              mmvae_stream_t stream);
int mmvae_normal_logratio_bwd(const float* packed_r, const float* z, const float* g, float* dpacked_r, int B, int D,
                              mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Reconstruction losses (per-sample sums), ReconLoss.* in models/objectives.py
 * ---------------------------------------------------------------------------------------------- */
/* bce (objectives.py:392-406) on x_hat = clamp(sigmoid(logit),1e-6,1-1e-6) (decoders.py:96-97):
 *   row_loss[b] = sum_f -[t log xh + (1-t) log(1-xh)];  x_hat (B,F) given (already clamped).
 * target_rows: the target has that many rows and row b of x_hat is compared with target row b % target_rows -- a
 * K-sample decoder output (K*B rows) against the target repeated K times (BaseObjective.reshape_for_loss,
 * objectives.py:118-120) without materialising the repeat; also in _sigmoid_clamp_bwd and ce_over_time_fwd / _bwd. */
int mmvae_bce_rowsum_fwd(const float* x_hat, const float* target, float* row_loss, int B, int F, int target_rows,
                         mmvae_stream_t stream);
/* dlogit[b,f] = g[b] * (xh - t) * [1e-6 < xh < 1-1e-6]  (gradient through sigmoid+clamp+bce) */
int mmvae_bce_sigmoid_clamp_bwd(const float* x_hat, const float* target, const float* g_row, float* dlogit,
                                int B, int F, int target_rows, mmvae_stream_t stream);
/* true gradient wrt x_hat: dxh[b,f] = g[b] * (xh - t) / max(xh (1 - xh), 1e-12)  (torch's bce backward) */
int mmvae_bce_rowsum_bwd(const float* x_hat, const float* target, const float* g_row, float* dxhat, int B, int F,
                         mmvae_stream_t stream);
/* backward of y = clamp(sigmoid(l), 1e-6, 1-1e-6): dl = dy * y (1 - y) * [1e-6 < y < 1-1e-6] */
int mmvae_sigmoid_clamp_bwd(const float* dy, const float* y, float* dl, long n, mmvae_stream_t stream);
/* elementwise bce (B,F) for the ReconLoss.bce API */
int mmvae_bce_elem_fwd(const float* x_hat, const float* target, float* loss, long n, mmvae_stream_t stream);

/* Loss terms whose upstream gradient is a known constant (the ELBO is linear in them: seed = llik_scaling / B):
 * row sums AND the logit gradient seed * d(row)/d(logit) from one pass, so the loss backward costs no launch.
 * bce: x_hat = clamp(sigmoid(logit)), dlogit = seed (x_hat - t) where the clamp is inactive.
 * ce_over_time: MMVAE_ERR_UNSUPPORTED when T*V > 4096 or V > 256 (use fwd + bwd). */
int mmvae_bce_rowsum_seeded(const float* x_hat, const float* target, float* row_loss, float seed, float* dlogit,
                            int B, int F, mmvae_stream_t stream);
int mmvae_ce_over_time_seeded(const float* logits, const float* target, float* row_loss, float seed, float* dlogits,
                              int B, int T, int V, mmvae_stream_t stream);

/* Element-wise forms of the loss-plugin contract `ReconLoss.<name>(output, target, bs) -> (bs, -1)`
 * (models/objectives.py:389-509); the mixers' objective() uses the per-sample row sums instead.
 * lprob (:409-424): out[i] = -log p(target[i % target_n]) under Normal / Laplace(loc[i], scale) as a DOUBLE (the
 *   reference casts the fp32 element), NaN -> 0 (no gradient); scale <= 0: scale := loc.  bwd: g (n doubles).
 * optimal_sigma (:503-509): out[i] = detach(((t - x) / sigma)^2) + log_sigma + log sqrt(2 pi), ONE log_sigma =
 *   softclip(log sqrt(mean (t - x)^2), -6) per call; stats (4 floats) = {mean square, log_sigma, raw log sigma};
 *   ws: mmvae_optimal_sigma_ws_floats(1, n) floats.  bwd: g (n floats), gradient through log_sigma only.
 * pointwise: kind 0 = l1 |x - t| (:427-442), 1 = mse (x - t)^2 (:444-459); row sums (target row b % target_rows) with
 *   their backward, and elements: mmvae_pointwise_elem writes the loss (g == NULL) or g * d loss / d x. */
int mmvae_lprob_elem_fwd(const float* loc, const float* target, double* out, long n, long target_n, float scale,
                         int laplace, mmvae_stream_t stream);
int mmvae_lprob_elem_bwd(const float* loc, const float* target, const double* g, float* dloc, long n, long target_n,
                         float scale, int laplace, mmvae_stream_t stream);
int mmvae_optimal_sigma_elem_fwd(const float* loc, const float* target, float* out, float* stats, float* ws, long n,
                                 mmvae_stream_t stream);
int mmvae_optimal_sigma_elem_bwd(const float* loc, const float* target, const float* g, const float* stats, float* ws,
                                 float* dloc, long n, mmvae_stream_t stream);
int mmvae_pointwise_rowsum_fwd(const float* x, const float* target, float* row_loss, int B, int F, int target_rows,
                               int kind, mmvae_stream_t stream);
int mmvae_pointwise_rowsum_bwd(const float* x, const float* target, const float* g_row, float* dx, int B, int F,
                               int target_rows, int kind, mmvae_stream_t stream);
int mmvae_pointwise_elem(const float* x, const float* target, const float* g, float* out, long n, int kind,
                         mmvae_stream_t stream);

/* category_ce (objectives.py:486-500): softmax over TIME.  logits/target (B,T,V) ->
 *   loss (B,V) = -sum_t tgt * log_softmax_t(logits);  row_loss[b] = sum_v loss[b,v]  (either may be NULL) */
int mmvae_ce_over_time_fwd(const float* logits, const float* target, float* loss, float* row_loss, int B, int T,
                           int V, int target_rows, mmvae_stream_t stream);
/* dlogits[b,t,v] = g[b,v] * (softmax_t(logits)[t] * sum_t' tgt[t'] - tgt[t]);  g (B,V) or g_row (B) */
int mmvae_ce_over_time_bwd(const float* logits, const float* target, const float* g, const float* g_row,
                           float* dlogits, int B, int T, int V, int target_rows, mmvae_stream_t stream);

/* ReconLoss.lprob (models/objectives.py:409-424): row[b] = sum_f -log p(target[b,f]) under Normal (laplace = 0) or
 * Laplace(loc[b,f], scale); elements in fp32, the row sum in fp64 (the reference sums the elements as doubles), NaN
 * elements count 0 and get zero gradient.  scale <= 0: scale := loc (BaseObjective.recon_loss_fn, objectives.py:43-45,
 * when the modality has masks).  target_rows: the target has that many rows and row b of loc is compared with target
 * row b % target_rows -- the K-sample case, where the reference repeats the target K times
 * (BaseObjective.reshape_for_loss, objectives.py:118-120); target_rows == B otherwise.  lap_block_rows > 0: `laplace`
 * is a bit mask over consecutive blocks of that many rows (bit j: rows [j, j+1) * lap_block_rows are Laplace) -- one
 * launch for a decoder pass whose own / cross reconstructions carry different likelihood families (MoE,
 * models/mmvae_models.py:101-103 vs :115); 0: `laplace` is the flag for every row.
 * perm_c > 0: loc (and dloc) are stored (B, perm_c, F / perm_c) -- the NCHW output of a conv decoder -- while element j
 * of a target row pairs with loc[b, j % perm_c, j / perm_c]: Dec_SVHN returns its output permuted to (B,H,W,C) and
 * the loss reshapes (does not permute) the NCHW target to that shape (decoders.py:144, objectives.py:120); the kernel
 * indexes instead of materialising the permuted copy.
 * logit_grad != 0: loc holds y = sigmoid(logits) written by the producing layer's epilogue, and bwd emits the
 * gradient with respect to the LOGITS, dloc = g * d(-log p)/dy * y (1 - y) (no separate sigmoid backward pass). */
int mmvae_lprob_rowsum_fwd(const float* loc, const float* target, float* row_loss, int B, int F, int target_rows,
                           float scale, int laplace, int lap_block_rows, int perm_c, mmvae_stream_t stream);
int mmvae_lprob_rowsum_bwd(const float* loc, const float* target, const float* g_row, float* dloc, int B, int F,
                           int target_rows, float scale, int laplace, int lap_block_rows, int perm_c, int logit_grad,
                           mmvae_stream_t stream);
/* ReconLoss.optimal_sigma (models/objectives.py:503-509) + utils.softclip (utils.py:66-69): one log sigma per call
 * from the mean squared error over all B*F elements; row[b] = sum_f ((t-x)/sigma)^2 + F (log sigma + log sqrt(2 pi)).
 * stats (3 floats, written by fwd, read by bwd) = {mean square, log sigma, unclipped log sigma}.  Gradient flows only
 * through log sigma (the squared term is detached in the reference). */
size_t mmvae_optimal_sigma_ws_floats(int B, int F);
int mmvae_optimal_sigma_fwd(const float* loc, const float* target, float* row_loss, float* stats, float* ws, int B,
                            int F, mmvae_stream_t stream);
int mmvae_optimal_sigma_bwd(const float* loc, const float* target, const float* g_row, const float* stats,
                            float* dloc, int B, int F, mmvae_stream_t stream);

/* out[k] = sum_n W[k,n] * sum_b V[n,b]   (ELBO assembly: BaseObjective.elbo objectives.py:54-67,
 * MoPOE.objective mmvae_models.py:315-319).  W is passed by value (<= 4 x 32 host floats). */
int mmvae_lincomb_rows_fwd(const float* V, const float* W_host, float* out, int n_rows, int B, int n_out,
                           mmvae_stream_t stream);
int mmvae_lincomb_rows_bwd(const float* gout, const float* W_host, float* dV, int n_rows, int B, int n_out,
                           mmvae_stream_t stream);

/* The same with the rows in separate tensors (p[n] -> B floats) and one upstream-gradient scalar per output
 * (g[k] device pointer or NULL = that output does not take part in backward); d rows are written to drows->p[n].
 * d_unit (may be NULL): fwd also writes the row gradients of output 0 for a unit upstream gradient (the constants
 * W[0][n]) -- a training step seeds loss.backward() with ones, so its backward needs no launch at all. */
typedef struct {
  const float* p[32];
} mmvae_rowptrs_t;
typedef struct {
  const float* g[4];
} mmvae_gptrs_t;
int mmvae_lincomb_rowptrs_fwd(const mmvae_rowptrs_t* rows, const float* W_host, float* out,
                              const mmvae_rowptrs_t* d_unit, int n_rows, int B, int n_out, mmvae_stream_t stream);
int mmvae_lincomb_rowptrs_bwd(const mmvae_gptrs_t* gout, const float* W_host, const mmvae_rowptrs_t* drows,
                              int n_rows, int B, int n_out, mmvae_stream_t stream);

/* MoE ELBO (models/mmvae_models.py:61-77): wc = exp(lw) * r;  loss = (sum_n W_n rowsum_n + n_nz beta sum kld) / M
 * where n_nz counts the rows whose weighted sum is not exactly 0 (the reference's `lp.sum() != 0` filter and the
 * broadcast in BaseObjective.elbo).  out (2 + n_rows floats): out[0] = loss, out[1] = n_nz, out[2 + n] = 1 if row n
 * is kept, else 0 (kept for the backward: a dropped row's gradient is 0). */
int mmvae_expmul_fwd(const float* lw, const float* r, float* out, int n, mmvae_stream_t stream);
int mmvae_expmul_bwd(const float* lw, const float* r, const float* g, float* dlw, float* dr, int n,
                     mmvae_stream_t stream);
int mmvae_moe_elbo_fwd(const float* rows, const float* W_host, const float* kld, float* out, int n_rows, int M, int B,
                       float beta, mmvae_stream_t stream);
int mmvae_moe_elbo_bwd(const float* g, const float* out, const float* W_host, float* drows, float* dkld, int n_rows,
                       int M, int B, float beta, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ResNet-50 image tower (`encoder: CNN`, models/encoders.py:86-127: torchvision resnet50 -> SiLU -> heads).  Inside the
 * tower activations are NHWC (rows = B*H*W, C) matrices; layers emit pre-activations, `in_act` (NONE / RELU) is applied
 * while reading.
 * ---------------------------------------------------------------------------------------------- */
/* AdaptiveAvgPool2d(1) on act(x): (B, HW, C) -> (B, C) */
int mmvae_avgpool_fwd(const float* x, float* y, int B, int HW, int C, int in_act, mmvae_stream_t stream);
int mmvae_avgpool_bwd(const float* dy, const float* x, float* dx, int B, int HW, int C, int in_act,
                      mmvae_stream_t stream);

/* ---- fused convolution + BatchNorm engine of the bottleneck stack (csrc/rconv.hip; replaces the reference's
 * torchvision Bottleneck.forward = conv1x1 -> bn -> relu -> conv3x3 -> bn -> relu -> conv1x1 -> bn (+ shortcut) and its
 * autograd backward, models/encoders.py:108).  Weights are channels-last: (Cout, T = k*k taps, Cin) in memory behind the
 * (Cout, Cin, k, k) parameter view.  A convolution's output stays RAW (pre-BatchNorm); its consumers apply
 * bn(y) = fma(y - mean, sc, beta), sc = gamma * rstd, and the ReLU while staging their LDS tiles.  `pre`: how the input is
 * consumed -- 0 as it is, 1 relu(x), 2 relu(bn(x)) with (xmean, xsc, xbeta).  All channel counts % 64 == 0. */
/* fwd (T, B*Ho*Wo) and bwd (T, B*H*W) int32 tables of a K x K / stride S / padding P convolution (-1 = no source) */
int mmvae_rc_tables(int* fwd, int* bwd, int B, int H, int W, int K, int S, int P, mmvae_stream_t stream);
/* rows per statistics partial the kernels use for an (M rows, N columns) output (64).  With R = ceil(M / 64) row tiles
 * a `part` buffer holds (R + ceil(R / 16)) * N * 2 floats and a `counter` buffer (N / 64) * (1 + ceil(R / 16)) tickets
 * (zero once; the kernels re-arm them): more than 16 row tiles elect their finalizer in two levels. */
int mmvae_rc_row_tile(int M, int N);
/* forward / data-gradient GEMMs with few output tiles split their reduction (K channels x T taps) over workgroups:
 * ws = mmvae_rc_conv_ws_floats(M, N, K, T) floats and (ceil(M / 64) + 4) * (N / 64) tile tickets (zero once) for an (M, N)
 * output (forward: N = Cout, K = Cin; data gradient: M = Min, N = Cin, K = Cout) */
int mmvae_rc_conv_splits(int M, int N, int K, int T);
size_t mmvae_rc_conv_ws_floats(int M, int N, int K, int T);
/* a BatchNorm whose output gradient a kernel produces: the kernel sums (G, G xhat) over the rows and its last workgroup
 * writes dgamma / dbeta ((+)= per acc) and pqr (3, C) with  dL/dY = G p + Y q + r  (torch.nn.BatchNorm2d backward,
 * training mode; eval: p = gamma rstd, q = r = 0) */
typedef struct {
  const float* Y;
  const float* mean;
  const float* rstd;
  const float* gamma;
  float* pqr;
  float* dgamma;
  float* dbeta;
  float* part;
  unsigned* counter;
  int acc;
  int eval;
} mmvae_rc_stat_t;
/* pixel geometry of a convolution: (B, H, W) input pixels -> (B, Ho, Wo) output pixels, KW columns of taps (T / KW rows),
 * stride S, padding P; H, W < 16384 */
typedef struct {
  int H, W, Ho, Wo, KW, S, P;
} mmvae_rc_geom_t;
/* forward: y (M, Cout) = conv(pre(x)); with part != NULL also the BatchNorm that follows: batch mean / rstd /
 * sc = gamma rstd out, running statistics moved (eval != 0: mean / rstd / sc from the running statistics, nothing moved) */
typedef struct {
  const float* x;
  const float* w;
  const float* xmean;
  const float* xsc;
  const float* xbeta;
  float* y;
  float* ws;
  unsigned* tile_ticket;
  int M, Cin, Cout, T, pre;
  mmvae_rc_geom_t g;
  const float* gamma;
  const float* beta;
  float* run_mean;
  float* run_var;
  float* mean;
  float* rstd;
  float* sc;
  float* part;
  unsigned* counter;
  float eps, momentum;
  int eval;
} mmvae_rc_fwd_t;
/* data gradient: out (Min, Cin) = mask * (conv_transpose(dY) + add), dY = G p + Y q + r per output channel (pqr NULL:
 * dY = G); add: (Min, Cin), or -- with add_tbl (Min) -- row add_tbl[m] of it (-1: none); mask: 0 none, 1 mY > 0,
 * 2 bn(mY) > 0 with (mmean, msc, mbeta); nstat BatchNorms (same rows / channels as out) get their backward
 * statistics from the epilogue */
typedef struct {
  const float* G;
  const float* Y;
  const float* pqr;
  const float* w;
  const float* add;
  const int* add_tbl;
  int mask;
  const float* mY;
  const float* mmean;
  const float* msc;
  const float* mbeta;
  float* out;
  float* ws;
  unsigned* tile_ticket;
  const int* row_map; /* stride 2, even H and W: the Min input pixels ordered by the parity class (ih % 2, iw % 2), classes
                         (0,0) (0,1) (1,0) (1,1), raster order inside a class -- a tile then only runs its class's taps
                         (9 / 4 instead of 9 passes per pixel for 3 x 3); statistics buffers sized for 4 * ceil(Min / 256)
                         row tiles.  NULL: raster order */
  int M, Min, Cin, Cout, T, nstat;
  mmvae_rc_geom_t g;
  mmvae_rc_stat_t st[2];
} mmvae_rc_dgrad_t;
/* weight gradient: dw (Cout, T, Cin) (+)= dY^T pre(x) per tap; tbl: the forward table of mmvae_rc_tables (NULL: 1x1,
 * stride 1); ws / counter: mmvae_rc_wgrad_ws_floats / _tickets */
typedef struct {
  const float* G;
  const float* Y;
  const float* pqr;
  const float* x;
  const float* xmean;
  const float* xsc;
  const float* xbeta;
  const int* tbl;
  float* dw;
  float* ws;
  unsigned* counter;
  int M, Cin, Cout, T, pre, accumulate;
} mmvae_rc_wgrad_t;
/* up to MMVAE_RC_MAX_JOBS independent jobs in ONE launch (a block's first convolution + projection shortcut, the
 * data gradients that only need one incoming gradient, batches of weight gradients beside the data-gradient chain);
 * kind: 0 forward (f), 1 data gradient (d), 2 weight gradient (w) */
#define MMVAE_RC_MAX_JOBS 8
typedef struct {
  int kind;
  mmvae_rc_fwd_t f;
  mmvae_rc_dgrad_t d;
  mmvae_rc_wgrad_t w;
} mmvae_rc_job_t;
int mmvae_rc_launch(const mmvae_rc_job_t* jobs, int n, mmvae_stream_t stream);
/* the same statistics for a gradient produced elsewhere (pooling backward) */
int mmvae_rc_bn_bwd_stats(const float* G, const mmvae_rc_stat_t* st, int M, int C, mmvae_stream_t stream);
/* ... and for the gradient of AdaptiveAvgPool2d(1) on relu(x) (torchvision resnet50.avgpool behind the last bottleneck),
 * made in the same launch: G (B*HW, C) = dy[b, c] / HW * (x > 0) */
int mmvae_rc_pool_bwd_stats(const float* dy, const float* x, float* G, const mmvae_rc_stat_t* st, int B, int HW, int C,
                            mmvae_stream_t stream);
int mmvae_rc_wgrad_splits(int M, int Cin, int Cout, int T);
size_t mmvae_rc_wgrad_ws_floats(int M, int Cin, int Cout, int T);
size_t mmvae_rc_wgrad_tickets(int Cin, int Cout, int T);
/* the stem (torchvision resnet50.conv1 / bn1 / relu / maxpool): y (M, Cout) = conv(img) of the NCHW image batch
 * (B, Cimg, H, W) with the channels-last weight (Cout, T, Cimg), BatchNorm statistics as in the forward jobs; max pooling
 * (3, 2, 1) of relu(bn(y)) with the index of each window's first maximum; its backward made in the launch that sums the
 * BatchNorm's backward statistics, G (B*H*W, C) = (bn(Y) > 0) * scattered dy (st->Y = y, st->mean with sc / beta
 * normalise); and the weight gradient, dY = G p + Y q + r, tbl (2, M): per output pixel b Cimg H W + h0 W + w0 and
 * (h0 + 16384) << 16 | (w0 + 16384) of its window origin (h0, w0) = (oh S - P, ow S - P). */
int mmvae_rc_stem_fwd(const float* img, const float* w, float* y, int M, int Cimg, int Cout, int T,
                      const mmvae_rc_geom_t* g, const float* gamma, const float* beta, float* run_mean, float* run_var,
                      float* mean, float* rstd, float* sc, float* part, unsigned* counter, float eps, float momentum,
                      int eval, mmvae_stream_t stream);
int mmvae_rc_maxpool_fwd(const float* y, const float* mean, const float* sc, const float* beta, float* out, int* idx, int B,
                         int H, int W, int C, mmvae_stream_t stream);
int mmvae_rc_maxpool_bwd_stats(const float* dy, const int* idx, float* G, const float* sc, const float* beta,
                               const mmvae_rc_stat_t* st, int B, int H, int W, int C, mmvae_stream_t stream);
int mmvae_rc_stem_wgrad_splits(int M, int Cimg, int Cout, int T);
size_t mmvae_rc_stem_wgrad_ws_floats(int M, int Cimg, int Cout, int T);
/* ws: mmvae_rc_stem_wgrad_ws_floats floats; counter: (Cout / 64) * ceil(T Cimg / 64) tickets (zero once) */
int mmvae_rc_stem_wgrad(const float* G, const float* Y, const float* pqr, const float* img, const int* tbl, float* dw,
                        float* ws, unsigned* counter, int M, int Cimg, int Cout, int T, const mmvae_rc_geom_t* g,
                        int accumulate, mmvae_stream_t stream);
/* end of a bottleneck: out = bn3(Y3) + (bn_d(R) when mr != NULL, else relu?(R)) */
int mmvae_rc_blockout(const float* Y3, const float* m3, const float* sc3, const float* b3, const float* R,
                      const float* mr, const float* scr, const float* br, int res_relu, float* out, long rows, int C,
                      mmvae_stream_t stream);
/* out = bn(Y) in the engine's own arithmetic (diagnostics, ReLU-mask export) */
int mmvae_rc_bn_apply(const float* Y, const float* mean, const float* sc, const float* beta, float* out, long rows, int C,
                      mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MoE with K samples per posterior + the DReG objective: the shipped configs/config_mnistsvhn.yml (mixing moe,
 * obj dreg, K 30, prior laplace).  Replaces MOE.forward's `q_m.rsample([K])` (models/mmvae_models.py:96-100),
 * the non-elbo branch of MOE.objective (:63-78) and MultimodalObjective.dreg / _m_dreg_looser
 * (models/objectives.py:361-387).
 *   packed[m] (B, 2D) = [mu_m | scale_m] head outputs (softmax + 1e-6 already applied); laplace[m] != 0: q_m is a
 *   Laplace (the config's `prior` key also selects the posterior family, models/trainer.py:104), else a Normal.
 *   eps[m] (K,B,D): standard Normal / Laplace variates (mmvae_randn / mmvae_rand_laplace);  z[m] (K,B,D) out.
 *   lat (M,K,B)   = sum_d log N(z_r[k,b]; 0, softmax(theta) D) - beta * log-mean-exp_m sum_d log q_m(z_r[k,b])
 *                   (beta = 1 for dreg, objectives.py:372; the objective's beta for iwae, objectives.py:356)
 *   pi  (M,K,B,M) = softmax_m of those row sums (saved for the backward pass).
 * bwd: dlat (M,K,B), dz[m] (K,B,D) or NULL -> dpacked[m] (B,2D) [written], dtheta_rows (B,D) [row b = sample b's
 *   contribution to d theta; the caller folds the rows; NULL = not wanted].  D <= 256, 2 <= M <= 4.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_MOE_MAX_MODS 4
typedef struct {
  const float* packed[MMVAE_MOE_MAX_MODS];
  const float* eps[MMVAE_MOE_MAX_MODS];
  float* z[MMVAE_MOE_MAX_MODS];
  int laplace[MMVAE_MOE_MAX_MODS];
} mmvae_moe_k_args;
typedef struct {
  const float* packed[MMVAE_MOE_MAX_MODS];
  const float* eps[MMVAE_MOE_MAX_MODS];
  const float* z[MMVAE_MOE_MAX_MODS];
  const float* dz[MMVAE_MOE_MAX_MODS];
  float* dpacked[MMVAE_MOE_MAX_MODS];
  int laplace[MMVAE_MOE_MAX_MODS];
} mmvae_moe_k_bwd_args;
int mmvae_moe_ksample_fwd(const mmvae_moe_k_args* a, const float* theta, float* lat, float* pi, int M, int K, int B,
                          int D, float beta, mmvae_stream_t stream);
int mmvae_moe_ksample_bwd(const mmvae_moe_k_bwd_args* a, const float* theta, const float* dlat, const float* pi,
                          float* dtheta_rows, int M, int K, int B, int D, float beta, mmvae_stream_t stream);
/* DReG loss (objectives.py:375-387).  own[r] / cross[r] (K*B): POSITIVE per-sample reconstruction sums of modality r
 * decoded from its own / the other modality's samples (mmvae_lprob_rowsum_fwd); lam[r] = llik_scaling.
 *   lw[r,k] = sum_b lat[r,k,b] - lam_r sum_b (own_r + cross_r)[k,b]   (fp64 sums);  w = softmax_k lw, detached;
 *   out (doubles, 1 + 2 M K + 2 M K): [0] loss = -(1/M) sum_rk w lw | lw (M,K) | w (M,K) | lpx (M,2,K) [own, cross]
 * bwd: g = d loss (device double) -> dlat (M,K,B) = -g w / M, d own = d cross = g w lam / M. */
typedef struct {
  const float* own[MMVAE_MOE_MAX_MODS];
  const float* cross[MMVAE_MOE_MAX_MODS];
  float lam[MMVAE_MOE_MAX_MODS];
} mmvae_dreg_rows;
typedef struct {
  float* own[MMVAE_MOE_MAX_MODS];
  float* cross[MMVAE_MOE_MAX_MODS];
  float lam[MMVAE_MOE_MAX_MODS];
} mmvae_dreg_rows_grad;
int mmvae_dreg_loss_fwd(const float* lat, const mmvae_dreg_rows* rows, double* out, int M, int K, int B,
                        mmvae_stream_t stream);
int mmvae_dreg_loss_bwd(const double* out, const double* g, const mmvae_dreg_rows_grad* rows, float* dlat, int M, int K,
                        int B, mmvae_stream_t stream);
/* IWAE loss (MultimodalObjective.iwae, objectives.py:342-359; the K > 1 AND B > 1 case is a defined extension, see
 * models/objectives.py of this package).  Same inputs as the DReG loss, per SAMPLE instead of summed over the batch:
 *   lw[r,k,b] = lat[r,k,b] - lam_r (own_r + cross_r)[k,b];  loss = -sum_b (logsumexp_{r,k} lw[.,.,b] - log(M K)), fp64
 *   out (doubles, mmvae_iwae_loss_out_doubles): [0] loss | lse (B) | lpx (M,2,K*B) [own, cross]
 * bwd: g = d loss (device double) -> dlat = -g softmax_{rk}(lw), d own = d cross = g softmax lam_r. */
size_t mmvae_iwae_loss_out_doubles(int M, int K, int B);
int mmvae_iwae_loss_fwd(const float* lat, const mmvae_dreg_rows* rows, double* out, int M, int K, int B,
                        mmvae_stream_t stream);
int mmvae_iwae_loss_bwd(const float* lat, const double* out, const double* g, const mmvae_dreg_rows_grad* rows,
                        float* dlat, int M, int K, int B, mmvae_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Enc_TxtRNN (models/encoders.py:840-869): Embedding -> bidirectional one-layer GRU(512) -> output[-1] -> sum of the
 * directions -> Linear -> chunk -> softmax + eta.  A DEFINED path, parity unpinned against the reference (its forward
 * crashes on its own batch format); oracle/mmvae_oracle.py: enc_txt_rnn, pinned to torch.nn.GRU.
 *   token_ids: onehot (B,T,V) -> ids (T,B) int32 [argmax; all-zero padding rows = token 0] + canonical one-hot (T*B,V).
 *   pt (3H,V) = W_ih E^T (the embedding folded into the input projection), bih / whh (3H,H) / bhh: torch's GRU
 *   parameters (gate order r, z, n).  forward: hs (T+1,B,H) with hs[0] = 0 given, hs[t+1] = h after step t (one launch
 *   per step: the (B,H)x(H,3H) product on 16x16x4 fp32 MFMA tiles with the gates in the epilogue);
 *   saved (4,T,B,H) = r | z | n | q (q = W_hn h + b_hn).  H % 64 == 0.
 *   backward: dh (B,H) = d loss / d h_T in (destroyed) -> dgx, dgh (T,B,3H): the input-side / hidden-side gate
 *   derivatives of every step (d Pt^T, d b_ih = reductions of dgx; d W_hh, d b_hh = reductions of dgh over hs[0:T]).
 *   cell0: the reverse direction at the last position = ONE cell step from h = 0 on the last token; out = hfwd + h;
 *   saved (3,B,H) = r | z | n;  bwd: dout (B,H) -> dgx, dgh (B,3H).
 * ---------------------------------------------------------------------------------------------- */
int mmvae_gru_token_ids(const float* onehot, int* ids, float* onehot_tb, int B, int T, int V, mmvae_stream_t stream);
int mmvae_gru_forward(const float* pt, const float* bih, const float* whh, const float* bhh, const int* ids, float* hs,
                      float* saved, int T, int B, int H, int V, mmvae_stream_t stream);
int mmvae_gru_backward(float* dh, const float* whh, const float* hs, const float* saved, float* dgx, float* dgh, int T,
                       int B, int H, mmvae_stream_t stream);
int mmvae_gru_cell0_fwd(const float* pt, const float* bih, const float* bhh, const int* ids, const float* hfwd,
                        float* out, float* saved, int B, int H, int V, mmvae_stream_t stream);
int mmvae_gru_cell0_bwd(const float* dout, const float* saved, const float* bhh, float* dgx, float* dgh, int B, int H,
                        mmvae_stream_t stream);

/* `prior: laplace` with the elbo objective: KL(Laplace(mu, s) || N(0,1)) row sums (torch's _kl_laplace_normal reached
 * through utils.kl_divergence, utils.py:399-402; models/mmvae_models.py:45) and the importance ratio of :56-62 under
 * Laplace posteriors (gradient into packed_r only, as mmvae_normal_logratio_*). */
int mmvae_kl_laplace_normal_fwd(const float* packed, float* kl, int B, int D, mmvae_stream_t stream);
int mmvae_kl_laplace_normal_bwd(const float* packed, const float* g, float* dpacked, int B, int D,
                                mmvae_stream_t stream);
int mmvae_laplace_logratio_fwd(const float* packed_r, const float* packed_o, const float* z, float* lw, int B, int D,
                               mmvae_stream_t stream);
int mmvae_laplace_logratio_bwd(const float* packed_r, const float* z, const float* g, float* dpacked_r, int B, int D,
                               mmvae_stream_t stream);
/* standard-Laplace variates e = -sign(u) log1p(-|u|), u ~ U(-1,1) (torch.distributions.Laplace.rsample: z = loc +
 * scale e); generator state as mmvae_randn */
int mmvae_rand_laplace(float* out, long n, uint32_t* state, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Held-out log-likelihood estimation (TorchMMVAE.estimate_log_likelihood; csrc/loglik.hip).  Forward only.
 * Mixture proposal q(z) = (1/C) sum_c q_c(z), q_c = Normal | Laplace(loc_c, scale_c) (bit c of laplace_mask), prior
 * p(z) = Normal | Laplace(prior_loc (D) or NULL = 0, softmax(theta) D).
 *   comps (C,B,2D) = [loc | scale] per component;  stratified: draw k0 + k comes from component (k0 + k) % C,
 *   z[k,b,:] = loc_c[b,:] + scale_c[b,:] * e[k,b,:]  (k = 0 .. Kc-1: chunk [k0, k0 + Kc) of a larger draw);
 *   e: eps (Kc,B,D) given, or eps = NULL and rng_state = the mmvae_randn / mmvae_rand_laplace generator state: element
 *   (k0 + k) B D + b D + d of the current draw of the component's family (the convention of mmvae_poe_reparam_kl_fwd),
 *   so a chunk repeats the matching slice of the whole draw; advance != 0: this launch bumps the call counter when it
 *   is done (pass it with the LAST chunk of a draw).
 *   lw0 (Kc,B) = sum_d log p(z[k,b,d]) - log((1/C) sum_c exp sum_d log q_c(z[k,b,d]))    (log-sum-exp form)
 * C <= MMVAE_MIX_MAX_COMPONENTS, D <= 256; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_MIX_MAX_COMPONENTS 8
int mmvae_mix_ksample_logw_fwd(const float* comps, unsigned laplace_mask, const float* theta, const float* prior_loc,
                               int prior_laplace, const float* eps, uint32_t* rng_state, int advance, float* z,
                               float* lw0, int C, int Kc, int k0, int B, int D, mmvae_stream_t stream);
/* Streaming log-sum-exp over the sample axis, fp64 sums.  state (1 + n_rows, 3, B) doubles, per (row, b): running
 * maximum | sum exp(w - max) | sum exp(2 (w - max)); an empty state is (-inf, 0, 0).  Row 0 holds the joint weights
 * w = lw0 + sum_{m: bit m of joint_mask} ll[m], row 1 + m the likelihood rows ll[m] themselves (lw0, ll[m]: (Kc,B)).
 * update folds one chunk of Kc samples into every row in one launch; finish (K = samples folded in all):
 *   out (1 + n_rows, B) = log-mean-exp_k,  ess (B) = exp(2 lse_k(w) - lse_k(2 w)) of row 0.
 * n_rows <= MMVAE_MOE_MAX_MODS. */
typedef struct {
  const float* ll[MMVAE_MOE_MAX_MODS];
} mmvae_lme_rows;
int mmvae_lme_update(double* state, const float* lw0, const mmvae_lme_rows* rows, int n_rows, unsigned joint_mask,
                     int Kc, int B, mmvae_stream_t stream);
int mmvae_lme_finish(const double* state, double* out, double* ess, int n_rows, long K, int B, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Latent classification (TorchMMVAE.classify_latents; csrc/probe.hip): linear probes on latent samples, the
 * reference's Latent_Classifier + CrossEntropyLoss + optim.Adam loop (eval/eval_mnistsvhn.py:24-67,
 * eval/mnistsvhn_helper.py:180-188).  Forward only for the model: no autograd.
 *   z (S,N,D) fp32: S packed latent matrices;  labels (A,N) int32: A label rows;
 *   probes: HOST pointer to (P,3) ints, probe p = (s_p, a_p, C_p): rows z[s_p], labels labels[a_p], C_p classes;
 *   state (P,3,Cmax (D+1)) fp32: per probe [parameters | exp_avg | exp_avg_sq], each a row-major (Cmax, D+1) matrix
 *   [W | b] (column D is the bias); classes >= C_p are never read or written.
 * mmvae_probe_train: one workgroup per probe runs the global steps [step0, step0 + n_steps).  Step t belongs to epoch
 *   e = t / ceil(N / batch) and covers the positions [i batch, min(N, (i + 1) batch)), i = t % ceil(N / batch), of that
 *   epoch (the last minibatch of an epoch may be short; its mean runs over the rows it has); position -> row through
 *   order (order_epochs, N) int32 (values in [0, N), row e is read for epoch e), or NULL = sequential.  Per step:
 *     logits = z_b W^T + b;  loss = mean_r (logsumexp_c logits - logits[label]);  dlogit = (softmax - onehot) / rows;
 *     dW = dlogit^T z_b, db = sum_r dlogit;  torch.optim.Adam defaults (betas 0.9 / 0.999, eps 1e-8, no amsgrad, no
 *     weight decay), bias corrections of step t + 1:  W -= lr / (1 - b1^(t+1)) * m / (sqrt(v) / sqrt(1 - b2^(t+1)) + eps).
 *   loss (P, n_steps): the mean loss of every step.  The state is read at the start of the launch and written at its end:
 *   a training split over launches at any step is bit-identical to one launch.  Every sum runs in a fixed order (no
 *   atomics): two runs are bit-identical, and a probe's result does not depend on the other probes of the launch.
 * mmvae_probe_eval: pred (P,N) int32 = argmax_c logits (the first maximum), nll (P,N) = the row's cross-entropy against
 *   labels[a_p] (labels may be NULL: nll is then 0 and a_p is not looked at).
 * D <= 256, 2 <= C_p <= Cmax <= MMVAE_PROBE_MAX_CLASSES, batch >= 1, 0 <= s_p < S, 0 <= a_p < A,
 * P <= MMVAE_PROBE_MAX_PROBES; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.  Labels outside [0, C_p)
 * are the caller's error (the Python binding raises ValueError before the launch).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_PROBE_MAX_CLASSES 32
#define MMVAE_PROBE_MAX_PROBES 64
int mmvae_probe_train(float* state, const float* z, const int* labels, const int* order, int order_epochs,
                      const int* probes, float* loss, int P, int S, int A, int N, int D, int Cmax, int batch, long step0,
                      int n_steps, float lr, mmvae_stream_t stream);
/* rows of the latent tile both kernels work on, a function of D alone (the order of the per-step loss sum follows it);
 * 0 for D outside 1 .. 256 */
int mmvae_probe_tile_rows(int D);
int mmvae_probe_eval(const float* state, const float* z, const int* labels, const int* probes, int* pred, float* nll,
                     int P, int S, int A, int N, int D, int Cmax, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Generation coherence (TorchMMVAE.cross_coherence / joint_coherence; csrc/coherence.hip): the scoring kernels of the
 * reference's eval/eval_cdsprites.py.  Forward only: no autograd.
 * mmvae_text_decode_score: logits (N,T,V) fp32 as Dec_TxtTransformer returns it (rows at padding all zero);
 *   pred (N,T) int32 = the index of the first maximum over V (torch.argmax on finite input; an all-zero row gives 0, the
 *   space of the alphabet);  with target_ids (N,T) int32 and lengths (N) int32:
 *   letters[n] = #{t < min(lengths[n], T) : pred[n,t] == target_ids[n,t]} (count_same_letters after its truncation to
 *   the shorter string; a negative length counts as 0).  target_ids NULL: only pred is written.
 *   1 <= T <= MMVAE_COH_MAX_STEPS, 2 <= V <= MMVAE_COH_MAX_VOCAB, else MMVAE_ERR_UNSUPPORTED.
 * mmvae_cls_head: the heads of A attribute classifiers (eval/train_classifiers.py: CNN) in one launch.
 *   feats (A,N,512): the fourth conv's output BEFORE its ReLU, flattened (channel, y, x);  W1 (A,256,512), b1 (A,256),
 *   W2 (A,Cmax,256), b2 (A,Cmax);  n_classes: HOST pointer to A ints.  Per classifier a:
 *     h = relu(relu(feats_a) W1_a^T + b1_a);  logits = h W2_a^T + b2_a over the first n_classes[a] classes;
 *     pred (A,N) int32 = the first maximum;  logits (A,N,Cmax) (may be NULL; columns >= n_classes[a] are written 0);
 *   with labels (A,N) int32: correct (A,N) uint8 = (labels >= 0 && pred == labels) -- a label of -1 ("the text names no
 *   value") is never correct -- and n_correct (N) int32 = sum_a correct[a,n] (zeroed on the stream, then integer
 *   atomics).  labels NULL: correct / n_correct are not touched.  Plain fp32 FMA accumulation in a fixed order; the
 *   hidden vector never leaves the registers.
 *   A <= MMVAE_COH_MAX_CLASSIFIERS, 2 <= n_classes[a] <= Cmax <= MMVAE_COH_MAX_CLASSES, else MMVAE_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_COH_MAX_STEPS 256
#define MMVAE_COH_MAX_VOCAB 256
#define MMVAE_COH_MAX_CLASSIFIERS 8
#define MMVAE_COH_MAX_CLASSES 8
#define MMVAE_COH_FEATS 512
#define MMVAE_COH_HIDDEN 256
int mmvae_text_decode_score(const float* logits, const int* target_ids, const int* lengths, int* pred, int* letters,
                            int N, int T, int V, mmvae_stream_t stream);
int mmvae_cls_head(const float* feats, const float* W1, const float* b1, const float* W2, const float* b2,
                   const int* n_classes, const int* labels, int* pred, float* logits, unsigned char* correct,
                   int* n_correct, int A, int N, int Cmax, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MNIST-SVHN digit coherence (TorchMMVAE.digit_cross_coherence / digit_joint_coherence; csrc/digits.hip): the
 * reference's two digit classifiers (eval/mnistsvhn_helper.py:191-226) and the loop that trains them
 * (eval/eval_mnistsvhn.py:70-120: CrossEntropyLoss + optim.Adam).  All fp32, no autograd.
 *   MMVAE_DIGIT_MNIST: x (1,28,28) -> conv1 1->10 k5 (10,24,24) -> maxpool 2 -> relu -> conv2 10->20 k5 (20,8,8)
 *     -> Dropout2d -> maxpool 2 -> relu -> flatten 320 (channel, y, x) -> fc1 320->50 -> relu -> dropout -> fc2 50->10
 *     -> log_softmax;  21 840 parameters.
 *   MMVAE_DIGIT_SVHN: x (3,32,32) -> (10,28,28) -> (10,14,14) -> (20,10,10) -> (20,5,5) = 500 -> 50 -> 10;  31 340.
 *   Packed parameters: conv1.w (10,C,5,5), conv1.b, conv2.w (20,10,5,5), conv2.b, fc1.w (50,flat), fc1.b, fc2.w (10,50),
 *   fc2.b, each in torch's layout.  state (nets,3,stride) fp32: per network [parameters | exp_avg | exp_avg_sq], stride >=
 *   the largest parameter count of the launch (elements past a network's count are never read or written).
 *   kinds: HOST pointer to `nets` ints;  images / labels: HOST arrays of `nets` DEVICE pointers, network i reads
 *   images[i] (N,C,H,W) fp32 and labels[i] (N) int32 (labels outside [0, 10) are the caller's error).
 *   Max-pool keeps the FIRST maximum of its window in row-major order and its backward sends the gradient there (torch's
 *   rule); ReLU's backward passes the gradient where the output is > 0.
 *   Dropout (training entry points only): mask element = 0 or 1 / (1 - p), drawn by the counter-based hash of
 *   csrc/common.hpp from (seed, kind, global step, position r of the row inside its minibatch, unit) and nothing else;
 *   Dropout2d masks the 20 channels of conv2's output, dropout the 50 outputs of relu(fc1).  p = 0: no dropout.
 * mmvae_digit_eval: logp (nets,N,10) log-probabilities, pred (nets,N) int32 = their first maximum; dropout off.
 * mmvae_digit_hidden: hidden (nets,N,50) = relu(fc1), the eval kernel's body up to that layer; dropout off.
 * mmvae_digit_grad: the first half of a training step on the minibatch images[i][0 .. rows): rowloss (nets,rows) =
 *   -logp[label], grad (nets,stride) = the gradient of mean_r rowloss with the masks of (seed, step).
 * mmvae_digit_train: the global steps [step0, step0 + n_steps), minibatch schedule and `order` (order_epochs, N) exactly
 *   as mmvae_probe_train (step t: positions [i batch, min(N, (i + 1) batch)) of epoch t / ceil(N / batch); the mean of a
 *   short last minibatch runs over the rows it has).  Per step two launches: one workgroup per (image, network) runs
 *   forward and backward and leaves the image's gradient in its row of ws; the second sums the rows -- four consecutive
 *   quarters of the minibatch, each in row order, added as (0 + 1) + (2 + 3) -- and applies torch.optim.Adam (defaults:
 *   betas 0.9 / 0.999, eps 1e-8, no amsgrad), bias corrections of step t + 1:
 *     p -= lr / (1 - b1^(t+1)) * m / (sqrt(v) / sqrt(1 - b2^(t+1)) + eps).
 *   loss (nets,n_steps): the mean loss of every step.  No atomics, every sum in a fixed order: two runs, one call or the
 *   same steps split over several, and a network trained alone or beside the other are bit-identical.
 *   ws: mmvae_digit_ws_floats(nets, batch, stride) floats (grad: batch = rows), private to the call until it has run.
 * mmvae_digit_masks: m2d (n_steps,batch,20) and m1 (n_steps,batch,50): the masks mmvae_digit_train / _grad use for the
 *   steps [step0, step0 + n_steps) of one network kind.
 * nets <= MMVAE_DIGIT_MAX_NETS, the two kinds, 0 <= p < 1, 1 <= batch, rows <= 65535; anything else returns
 * MMVAE_ERR_UNSUPPORTED and writes nothing.  The row cap is a budget, not an index limit: ws holds one gradient row of
 * stride floats per image of the minibatch, 8.2 GB per network at 65535 rows of 31340.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_DIGIT_MNIST 0
#define MMVAE_DIGIT_SVHN 1
#define MMVAE_DIGIT_MAX_NETS 2
int mmvae_digit_n_params(int kind); /* 21840 / 31340; 0 for an unknown kind */
size_t mmvae_digit_ws_floats(int nets, int batch, int stride);
int mmvae_digit_eval(const float* state, const int* kinds, const float* const* images, float* logp, int* pred, int nets,
                     int stride, long N, mmvae_stream_t stream);
int mmvae_digit_hidden(const float* state, const int* kinds, const float* const* images, float* hidden, int nets,
                       int stride, long N, mmvae_stream_t stream);
int mmvae_digit_grad(const float* state, const int* kinds, const float* const* images, const int* const* labels,
                     float* ws, float* grad, float* rowloss, int nets, int stride, int rows, unsigned seed, long step,
                     float p, mmvae_stream_t stream);
int mmvae_digit_train(float* state, const int* kinds, const float* const* images, const int* const* labels,
                      const int* order, int order_epochs, float* ws, float* loss, int nets, int stride, int N, int batch,
                      long step0, int n_steps, float lr, unsigned seed, float p, mmvae_stream_t stream);
int mmvae_digit_masks(float* m2d, float* m1, int kind, unsigned seed, long step0, int n_steps, int batch, float p,
                      mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Latent analysis (TorchMMVAE.analyse_latents; csrc/tsne.hip): the exact t-SNE embedding of the latent samples, which the
 * reference draws with sklearn.manifold.TSNE on 250 samples per modality (visualization.py: t_sne, called from
 * models/trainer.py:242-272).  The arithmetic is scikit-learn's method="exact" path; eps = 2.220446049250313e-16.
 *   mmvae_tsne_sqdist: D2 (N,N) fp32, D2[i,j] = sum_d (x_id - x_jd)^2 summed directly in double (no Gram trick) and
 *     rounded to fp32; zero diagonal, symmetric bit for bit.
 *   mmvae_tsne_joint_p: per row the binary search of _binary_search_perplexity in double (beta = 1, bracket (-inf, inf),
 *     at most 100 steps; p_j = exp(-D2[i,j] beta), s = sum_{j != i} p_j, s = 1e-8 if s == 0, H = log s + beta sum_j D2[i,j]
 *     p_j / s, stop at |H - log perplexity| <= 1e-5, else double / halve beta or take the midpoint of the bracket);
 *     info (N,4) doubles = the beta the returned row was computed with, its s, sum_j p_j / s, the steps taken.
 *     P (N, ldp) fp32, ldp = mmvae_tsne_ld(N) (N rounded up to 4; the pad columns are written 0):
 *     P_ij = max((c_ij + c_ji) / max(sum, eps), eps), c_ij = p_j / s of row i, P_ii = 0; sum = 2 sum_i info[i,2] reduced in a
 *     fixed order into total[0].  Symmetric bit for bit.
 *   One iteration `it` (0-based): ex = 12, momentum 0.5 for it < switch_it (scikit-learn: 250), then 1 and 0.8;
 *     w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij, g_i = 4 sum_j (ex P_ij - w_ij / Z) w_ij (y_i - y_j),
 *     KL = sum_{i != j} ex P_ij log(max(ex P_ij, eps) Z / w_ij); gains += 0.2 where upd g < 0, *= 0.8 elsewhere, >= 0.01;
 *     upd = momentum upd - lr gains g; y += upd.  (Q_ij = w_ij / Z without scikit-learn's clamp at eps: the two differ
 *     only for pairs with w_ij / Z < eps.)  Pair terms in fp32, every sum over pairs accumulated in double.
 *   state (3,N,2) fp32 = Y | upd | gains; ws: mmvae_tsne_ws_doubles(N) doubles, private to the call until it has run.
 *   mmvae_tsne_forces: the first half of iteration `it`: g (N,2) fp32, kz = (KL, Z) doubles; the state is not written.
 *   mmvae_tsne_run: the iterations [it0, it0 + n_iter), two launches each; log (n_iter,2) doubles = (KL, |g|_2) of every
 *     iteration, KL only where (it + 1) % kl_every == 0 (NaN elsewhere: the logarithms are the costly part of a pair).
 *   No atomics, every sum in a fixed order: two runs, and one call or the same iterations split over several, are
 *   bit-identical.  MMVAE_TSNE_MIN_POINTS <= N <= MMVAE_TSNE_MAX_POINTS (P is 1 GB there), D <= MMVAE_TSNE_MAX_DIM;
 *   anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_TSNE_MAX_POINTS 16384
#define MMVAE_TSNE_MAX_DIM 256
#define MMVAE_TSNE_MIN_POINTS 4
int mmvae_tsne_ld(int N); /* 0 for N outside the limits */
size_t mmvae_tsne_ws_doubles(int N);
int mmvae_tsne_sqdist(const float* X, float* D2, int N, int D, mmvae_stream_t stream);
int mmvae_tsne_joint_p(const float* D2, double perplexity, float* P, int ldp, double* info, double* total, int N,
                       mmvae_stream_t stream);
int mmvae_tsne_forces(const float* state, const float* P, int ldp, double* ws, float* g, double* kz, int N, long it,
                      long switch_it, mmvae_stream_t stream);
int mmvae_tsne_run(float* state, const float* P, int ldp, double* ws, double* log, int N, long it0, int n_iter,
                   long switch_it, double lr, int kl_every, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Frechet distance of generated images (TorchMMVAE.frechet_distances; csrc/frechet.hip): the arithmetic of the
 * reference's calculate_frechet_distance (eval/fid_score.py:203-257),
 *   d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2,
 * over feature vectors, everything in double, no atomics, every sum in a fixed order: two runs give the same bits.
 *   Moments, streaming.  state: mmvae_frechet_state_doubles(F) = 1 + F + F F doubles = n | mean (F) | M2 (F,F), all 0
 *     before the first batch.  mmvae_frechet_update folds X (nb,F) fp32: the batch mean (rows summed in double: four
 *     consecutive quarters, each in row order, added as (0 + 1) + (2 + 3)), the centred scatter sum_r (x_r - mean_b)
 *     (x_r - mean_b)^T as one tiled SYRK on v_mfma_f64_16x16x4_f64 (rows converted and centred in double on load; the
 *     tiles on and above the diagonal are computed, the others mirrored; k runs over the rows in order, no K-split), and
 *     Chan's merge in its epilogue: delta = mean_b - mean, M2 += scatter + delta delta^T n nb / (n + nb), then
 *     mean += delta nb / (n + nb), n += nb.  ws: F doubles.  Memory does not grow with the number of rows.
 *     mmvae_frechet_finish: mu = mean, sigma = M2 / (n - 1) (np.cov); n is the caller's copy of state[0], n >= 2.
 *   mmvae_f64_gemm: C = A B (trans_b = 0) or A B^T on row-major (F,F) doubles, the same MFMA tile routine (64 x 64 per
 *     workgroup, k in steps of 4 in order); C must not alias A or B.
 *   mmvae_sym_eig: one-sided (Hestenes) Jacobi on A <- S (symmetric, row-major: its rows are the columns the sweeps
 *     rotate), V <- I.  Round-robin ordering over n = F + (F odd) columns: a sweep is n - 1 steps of n / 2 disjoint
 *     pairs, pair k of step s = (n - 1, s) for k = 0, ((s + k) mod (n - 1), (s - k) mod (n - 1)) for k >= 1; a pair that
 *     touches the padding column F is skipped.  One launch per step; one wave per pair for F <= 256, one workgroup of
 *     four waves above (mmvae_sym_eig_waves_per_pair).  Per pair a = |A_p|^2, b = |A_q|^2, c = A_p . A_q (per-thread
 *     strided partials, a shuffle butterfly, four waves added as (0 + 1) + (2 + 3)); rotate when c != 0 and
 *     c^2 > 1e-30 a b: zeta = (b - a) / (2 c), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (0 when zeta overflows),
 *     cs = 1 / sqrt(1 + t^2), sn = cs t, (A_p, A_q) <- (cs A_p - sn A_q, sn A_p + cs A_q), the same on V.  A rotation is
 *     COUNTED only when a and b both exceed floor^2 = (F 2^-52 max_j |S_j|)^2 (a zero row of S never converges by the
 *     relative rule alone); the sweeps stop after the first one without a counted rotation.  The host reads one
 *     integer per sweep (the call synchronises the stream).  Reaching max_sweeps <= MMVAE_EIG_MAX_SWEEPS returns
 *     MMVAE_ERR_NO_CONVERGENCE.  values (F) = |A_j| (the eigenvalues of a positive semi-definite S, in no particular
 *     order); Vc (F,F) or NULL (values only: the same rotations, the same bits): Vc[j F + i] = V[i][j], column j the
 *     eigenvector of values[j]; sweeps, rotations (max_sweeps): HOST ints, the sweeps run and the counted rotations of
 *     each.  ws: mmvae_sym_eig_ws_doubles(F) = F F + 2 F + 64 doubles.
 *   mmvae_frechet_distance: (lambda, V) of sigma1; R = diag(sqrt(lambda)) V^T; T = sigma2 R^T; G = R T; the singular
 *     values of G, values only; tr (S1 S2)^1/2 = sum_j sqrt(sigma_j(G)).  out (5) doubles on the device = d^2,
 *     tr covmean, |mu1 - mu2|^2, tr S1, tr S2 (thread t of 256 sums the terms t, t + 256, ..., the partials are added in
 *     thread order); sweeps (2): HOST ints.  ws: mmvae_frechet_ws_doubles(F) = mmvae_sym_eig_ws_doubles(F) + 2 F F + 2 F.
 *   1 <= F <= MMVAE_FRECHET_MAX_F, nb >= 1, n >= 2; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.  The
 *   size helpers are host functions (0 outside the limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_FRECHET_MAX_F 2048
#define MMVAE_EIG_MAX_SWEEPS 30
size_t mmvae_frechet_state_doubles(int F);
size_t mmvae_sym_eig_ws_doubles(int F);
size_t mmvae_frechet_ws_doubles(int F);
int mmvae_sym_eig_waves_per_pair(int F); /* 1 or 4; 0 outside the limits */
int mmvae_frechet_update(double* state, const float* X, double* ws, long nb, int F, mmvae_stream_t stream);
int mmvae_frechet_finish(const double* state, double* mu, double* sigma, long n, int F, mmvae_stream_t stream);
int mmvae_f64_gemm(const double* A, const double* B, double* C, int F, int trans_b, mmvae_stream_t stream);
int mmvae_sym_eig(const double* S, double* ws, double* Vc, double* values, int* sweeps, int* rotations, int F,
                  int max_sweeps, mmvae_stream_t stream);
int mmvae_frechet_distance(const double* mu1, const double* sigma1, const double* mu2, const double* sigma2, double* ws,
                           double* out, int* sweeps, int F, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * k-nearest-neighbour manifold estimates of generated images (TorchMMVAE.manifold_metrics; csrc/manifold.hip): improved
 * precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020).  Feature rows are fp32,
 * squared distances are taken in double through the Gram product:
 *   n2[i] = sum_f x_if^2 (f in order, one thread per row), g_ij = sum_f b_if a_jf, d^2_ij = max(0, (n2_i + n2_j) - 2 g_ij).
 *   g is one tiled product on v_mfma_f64_16x16x4_f64 (rows converted to double on load; 64 x 64 tile per workgroup; f
 *   walked in order in steps of 4, no split over F: one summation order per g_ij, the same for (i,j) and (j,i)).  The
 *   rows x cols matrix is never written: a workgroup owns 64 rows and a chunk of column tiles and reduces every tile in
 *   its epilogue; the chunks' partials of a row go to ws and a second launch merges them in chunk order.  No atomics;
 *   integer sums, minima and "the k smallest" do not depend on the split: two runs and any two plans give the same bits.
 *   mmvae_manifold_sqnorms: n2 (rows) doubles.
 *   mmvae_manifold_radii: rad2[i] = the k-th smallest d^2(X_i, X_j) over j != i, the row itself left out by INDEX (a
 *     duplicate row is an ordinary neighbour at distance 0); rows >= k + 1.
 *   mmvae_manifold_cross: query rows B against manifold rows A with their rad2_a: count[j] (int32) = #{i : d^2(B_j, A_i)
 *     <= rad2_a[i]} (a point on a sphere is inside), mind2[j] = min_i d^2(B_j, A_i).  (B, A) = (generated, real) gives the
 *     hits behind precision and density, (real, generated) those behind recall and the distances behind coverage.
 *   chunks: 0 = the default plan, mmvae_manifold_chunks(rows, cols) = min(ceil(512 / row tiles), ceil(column tiles / 4))
 *     chunks (two workgroups per CU of 256 at 10 000 rows, at least four column tiles per chunk); a positive value asks
 *     for that many (at most one per column tile).  Chunk c holds the column tiles [c t, (c + 1) t), t = ceil(column
 *     tiles / chunks); chunks that would be empty are not launched.
 *   ws: mmvae_manifold_ws_doubles(rows, cols, k, chunks) = launched chunks x rows x max(k, 2) doubles; radii: (chunk, row,
 *     k) the chunk's k smallest ascending, +inf where it met fewer; cross (k = 1): (chunk, row, 2) = (count, smallest d^2).
 *   1 <= rows <= MMVAE_MANIFOLD_MAX_ROWS, 1 <= k <= MMVAE_MANIFOLD_MAX_K, 1 <= F <= MMVAE_FRECHET_MAX_F, chunks >= 0;
 *   anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.  The size helpers are host functions (0 outside the
 *   limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_MANIFOLD_MAX_ROWS 16384
#define MMVAE_MANIFOLD_MAX_K 16
int mmvae_manifold_chunks(long rows, long cols);
size_t mmvae_manifold_ws_doubles(long rows, long cols, int k, int chunks);
int mmvae_manifold_sqnorms(const float* X, double* n2, long rows, int F, mmvae_stream_t stream);
int mmvae_manifold_radii(const float* X, const double* n2, double* ws, double* rad2, long rows, int F, int k, int chunks,
                         mmvae_stream_t stream);
int mmvae_manifold_cross(const float* B, const double* nb, const float* A, const double* na, const double* rad2_a,
                         double* ws, int* count, double* mind2, long rows_b, long rows_a, int F, int chunks,
                         mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Aggregate posterior of the latent code (TorchMMVAE.disentanglement; csrc/aggpost.hip): what the ELBO decomposition
 * (index-code mutual information, total correlation, dimension-wise KL; Chen et al. 2018) and the mutual information gap
 * read.  z, loc, scale (N,D) fp32, row n of z a draw from posterior n; labels (K,N) int32 >= 0 or NULL with K = 0.  Pair
 * term in double from the fp32 inputs converted on load, t = (z_nd - loc_md) / s_md (as a product with 1 / s_md):
 *   Normal (laplace 0)  l[n,m,d] = -t^2 / 2 - log s_md - log(2 pi) / 2        Laplace  l[n,m,d] = -|t| - log(2 s_md)
 *   joint[n]           = logsumexp_m sum_d l[n,m,d] - log N                                      (N)     doubles
 *   marginal[n,d]      = logsumexp_m l[n,m,d] - log N                                            (N,D)   doubles
 *   conditional[k,n,d] = logsumexp_{m : labels[k,m] == labels[k,n]} l[n,m,d] - log N_c           (K,N,D) doubles,
 *     N_c the size of that class, counted inside the launch.
 *   A fixed shift, no running maximum: row n is one of the m (of its own class too), so that sum_m exp(l[n,m,d] -
 *   l[n,n,d]) holds the term 1; its argument is at most the row's own standardised residual plus log(s_n / s_m), hundreds
 *   of nats below the overflow at 709 for a z drawn from its posterior, and terms below -745 vanish.  Every accumulator
 *   is a plain fp64 sum of exp(l - shift), chunks merge by addition, the result is shift + log(sum) - log(count).  (A z
 *   thousands of deviations from its own posterior overflows the sum: the outputs are +inf there, never a wrong number.)
 *   Four launches: the shifts l[n,n,d] and sum_d l[n,n,d] (d in order); the (n,d) sums -- a workgroup owns 64 sample rows
 *   (one per lane), 16 dimensions (4 per wave) and a chunk of posterior rows staged 32 at a time in LDS as (loc, 1 / s,
 *   -log s - const) beside their labels: one exp per (n,m,d), the K class sums reuse it through a select --; the joint
 *   sums -- the same rows and chunk, a thread adds l over d in order in a register per pair and takes one exp per (n,m),
 *   and counts the classes --; the merge of the chunks' partials in chunk order.  The N x N x D terms are never written;
 *   no atomics; two runs with one plan give the same bits, two plans regroup fp64 sums.
 *   chunks: 0 = the default plan, mmvae_aggpost_chunks(N, D) = min(ceil(2048 / (ceil(N / 64) ceil(D / 16))), ceil(tiles
 *     / 2)) chunks, tiles = ceil(N / 32) staged tiles; a positive value asks for that many (at most one per tile).  Chunk
 *     c holds the tiles [c t, (c + 1) t), t = ceil(tiles / chunks); chunks that would be empty are not launched.
 *   ws: mmvae_aggpost_ws_doubles(N, D, K, chunks) doubles = shift (N,D) | joint shift (N) | (chunk, n, d, 1 + K) sums,
 *     all rows first, then per factor | (chunk, n, 1 + K) joint sum, then the class members met per factor.
 *   1 <= N <= MMVAE_AGGPOST_MAX_ROWS, 1 <= D <= 256, 0 <= K <= MMVAE_AGGPOST_MAX_FACTORS, chunks >= 0; anything else
 *   returns MMVAE_ERR_UNSUPPORTED and writes nothing.  The two helpers are host functions (0 outside the limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_AGGPOST_MAX_ROWS 16384
#define MMVAE_AGGPOST_MAX_FACTORS 8
int mmvae_aggpost_chunks(long N, int D);
size_t mmvae_aggpost_ws_doubles(long N, int D, int K, int chunks);
int mmvae_aggpost_lse(const float* z, const float* loc, const float* scale, int laplace, const int* labels, double* ws,
                      double* joint, double* marginal, double* conditional, long N, int D, int K, int chunks,
                      mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Kernel inception distance of generated images (TorchMMVAE.kernel_distances; csrc/kid.hip): the sums behind the unbiased
 * MMD^2 (Binkowski et al. 2018) under the polynomial kernel k(x, y) = (gamma x . y + coef0)^degree, over `subsets` random
 * subsets of m rows.  X (rows_x, F) and Y (rows_y, F) are fp32 feature rows; idx_x, idx_y (subsets, m) int32 list, per
 * subset, the rows taken from X and from Y: x_i = X[idx_x[s, i]], y_j = Y[idx_y[s, j]].  sums (subsets, 3) doubles:
 *   sums[s, 0] = sxx = sum_{i != j} k(x_i, x_j)      sums[s, 1] = syy = sum_{i != j} k(y_i, y_j)
 *   sums[s, 2] = sxy = sum_{i, j} k(x_i, y_j)
 *   The diagonal of sxx and syy is left out by POSITION i == j in the list (a row number that a list repeats is an
 *   ordinary pair); sxy holds all m^2 terms.  MMD^2[s] = (sxx + syy) / (m (m - 1)) - 2 sxy / m^2 is the caller's.
 *   g_ij = x_i . y_j is the tiled product of csrc/manifold.hip on v_mfma_f64_16x16x4_f64 (64 x 64 tile per workgroup; f
 *   walked in order in steps of 4, no split over F), its rows converted to double on load and addressed through the
 *   index list in the fetch: no gathered copy of the rows exists.  Epilogue per element: t = gamma g + coef0, t^degree by
 *   degree - 1 successive products by t; four threads per row add the tile's values of their row.  The m x m block is
 *   never written.  One launch, grid (chunks, row tiles, 3 subsets), covers every (subset, pair) slice; sxx and syy walk
 *   only the column tiles on or above the diagonal tile and count the tiles strictly above it twice (a product by 2 is
 *   exact).  A second launch adds the row partials of a slice in a fixed order.  No atomics: for a given (m, chunks) two
 *   runs give the same bits; two chunk plans regroup fp64 sums and agree to rounding only.
 *   THE DEVICE DOES NOT CHECK THE INDICES: every idx_x[s, i] must lie in [0, rows_x), every idx_y[s, j] in [0, rows_y)
 *   (ops.kid_sums checks before every call).
 *   chunks: 0 = the default plan, mmvae_kid_chunks(subsets, m) = min(ceil(512 / (3 subsets tiles)), ceil(tiles / 4))
 *     chunks, tiles = ceil(m / 64) (two workgroups per CU of 256, at least four column tiles per chunk: 1 chunk from 3
 *     subsets of 1000 rows on); a positive value asks for that many (at most one per column tile).  Chunk c holds the
 *     column tiles [c t, (c + 1) t), t = ceil(tiles / chunks); chunks that would be empty are not launched.
 *   ws: mmvae_kid_ws_doubles(subsets, m, chunks) = 3 subsets x launched chunks x m doubles, (slice, chunk, position).
 *   2 <= m <= MMVAE_KID_MAX_SUBSET, 1 <= subsets <= MMVAE_KID_MAX_SUBSETS, 1 <= F <= MMVAE_FRECHET_MAX_F, 1 <= degree <=
 *   MMVAE_KID_MAX_DEGREE, rows_x, rows_y >= 1, chunks >= 0; anything else returns MMVAE_ERR_UNSUPPORTED and writes
 *   nothing.  The two helpers are host functions (0 outside the limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_KID_MAX_SUBSET 16384
#define MMVAE_KID_MAX_SUBSETS 1024
#define MMVAE_KID_MAX_DEGREE 8
int mmvae_kid_chunks(int subsets, long m);
size_t mmvae_kid_ws_doubles(int subsets, long m, int chunks);
int mmvae_kid_sums(const float* X, const float* Y, const int* idx_x, const int* idx_y, double* ws, double* sums,
                   long rows_x, long rows_y, int F, int subsets, long m, int degree, double gamma, double coef0, int chunks,
                   mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Kernel two-sample test of latents (TorchMMVAE.latent_two_sample; csrc/mmd.hip): the sums behind the unbiased MMD^2
 * (Gretton et al. 2012) of X (n_x, D) against Y (n_y, D), fp32 rows, for the observed split and for P relabellings of the
 * pooled sample (X's rows, then Y's; n = n_x + n_y).  member (P, n) bytes: row p marks with 1 the pooled rows that count as
 * "X" under relabelling p (n_x ones per row: the caller checks; NULL with P = 0).  With d^2 = |x - y|^2:
 *   MMVAE_MMD_RBF     k = (1 / S) sum_s exp(-params[s] d^2)             (params: the S rates gamma_s)
 *   MMVAE_MMD_IMQ     k = (1 / S) sum_s params[s] / (params[s] + d^2)   (params: the S constants c_s)
 *   MMVAE_MMD_ENERGY  k = -d                                            (params and S are not read)
 * params is a HOST array of S finite positive doubles (anything else: MMVAE_ERR_ARG).
 *   sums (1 + P, 3) doubles: row 0 the observed split, row 1 + p relabelling p, each
 *     [sum_{i != j, both X} k_ij, sum_{i != j, both Y} k_ij, sum_{i in X, j in Y} k_ij]   (the layout of mmvae_kid_sums)
 *   row_sums (n) doubles: r_i = sum_{j != i} k_ij.  The diagonal is left out by POSITION.
 *   Arithmetic: rows centred by the pooled mean in double (the families are translation invariant), d^2 = max(0, (|z_i|^2
 *   + |z_j|^2) - 2 z_i . z_j) with the Gram tiles of csrc/pair_tile.hpp on v_mfma_f64_16x16x4_f64 and |z_i|^2 taken from
 *   the diagonal of the same tiles; a pair whose d^2 comes out below a quarter of |z_i|^2 + |z_j|^2 (the Gram form has
 *   cancelled: close rows of a wide sample) is computed again by differences, so rows with equal bits give d = 0 exactly
 *   and clusters far apart cost no accuracy.  Per split with indicator a: r = K 1,
 *   T = 1' r, sxx = a' K a, sxy = (1 - a)' K a, each a sum of its own terms, syy = (T - sxx) - 2 sxy.  K a: every 64 x 64
 *   tile of K, in LDS, times
 *   the 64 x MMVAE_MMD_PBLOCK block of indicator columns (column 0 the observed split, 1 + p relabelling p) on the same
 *   MFMA, dotted with the row tile's indicators (and their complement) and summed over a chunk of column tiles; blocks of columns are on the grid
 *   and the first of them also adds the rows of every tile (r).  The n x n matrix is never written.  Three small launches merge the partials in a fixed order.  No atomics: two runs with one plan give the
 *   same bits, a split's row does not depend on its position in `member` or on P; two chunk plans agree to rounding only.
 *   chunks: 0 = the default plan, mmvae_mmd_chunks(n) = min(ceil(512 / tiles), ceil(tiles / 4)), tiles = ceil(n / 64) (a
 *     function of n alone); a positive value asks for that many (at most one per column tile).
 *   ws: mmvae_mmd_ws_doubles(n, D, P, chunks) doubles (centred rows, norms, partials, packed indicators).
 *   2 <= n_x, n_y, n <= MMVAE_MMD_MAX_ROWS, 1 <= D <= MMVAE_MMD_MAX_D, 0 <= P <= MMVAE_MMD_MAX_PERMUTATIONS, 1 <= S <=
 *   MMVAE_MMD_MAX_SCALES, chunks >= 0; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.  The two helpers
 *   are host functions (0 outside the limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_MMD_MAX_ROWS 16384
#define MMVAE_MMD_MAX_D 256
#define MMVAE_MMD_MAX_PERMUTATIONS 2048
#define MMVAE_MMD_MAX_SCALES 8
#define MMVAE_MMD_PBLOCK 128
#define MMVAE_MMD_RBF 0
#define MMVAE_MMD_IMQ 1
#define MMVAE_MMD_ENERGY 2
int mmvae_mmd_chunks(long n);
size_t mmvae_mmd_ws_doubles(long n, int D, int P, int chunks);
int mmvae_mmd_sums(const float* X, const float* Y, const unsigned char* member, double* ws, double* sums, double* row_sums,
                   long n_x, long n_y, int D, int P, int family, const double* params, int S, int chunks,
                   mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sliced Wasserstein distances and marginal Kolmogorov-Smirnov tests (ops.swd_slices, TorchMMVAE.latent_transport and
 * sliced_distances; csrc/swd.hip): X (n_x, F) and Y (n_y, F) fp32 rows are projected on L directions, every projection is
 * sorted, and the two sorted lists of a direction are compared.  dirs (L, F) doubles on the device; dirs NULL selects AXIS
 * MODE: L must equal F (<= MMVAE_SWD_MAX_DIRECTIONS) and direction d is coordinate d -- the projection is the float
 * converted to double, no multiplication, exact.  Per direction l, with x_(0) <= ... <= x_(n_x - 1), y_(0) <= ... <=
 * y_(n_y - 1) the sorted projections and N = n_x n_y:
 *   w (L, 2) doubles: w[l][0] = W_1, w[l][1] = W_2^2 of the two empirical measures, exact for unequal sizes: the quantile
 *     functions are steps on a grid of 1 / N, x_(i) covers [i n_y, (i + 1) n_y), y_(j) covers [j n_x, (j + 1) n_x), and
 *     W_p^p = (1 / N) sum over overlapping (i, j) of len_ij |x_(i) - y_(j)|^p, len_ij the integer overlap.  Order of the sum:
 *     thread t of 1024 adds the terms of i = t, t + 1024, ... with i ascending and j ascending within i; the 1024 partials are
 *     added by the tree p[t] += p[t + o] for o = 512, 256, ..., 1; one division by N.
 *   ks (L) 64-bit integers: the numerator of the two-sample Kolmogorov-Smirnov statistic, max over the pooled values t of
 *     |n_y #{x <= t} - n_x #{y <= t}| (D = ks / N), taken at the last element of every run of equal values: exact under ties.
 *   Projections: the tile routine of mmvae_f64_gemm on v_mfma_f64_16x16x4_f64 (directions as doubles, rows converted on
 *     load), k in steps of 4 in order, no K-split: the bits of a projection depend on its row and its direction only -- not on
 *     L, on the direction's place among the directions, on n_x or n_y; rows with equal bits project to equal bits in
 *     whichever set they sit.
 *   Sort: one workgroup per (direction, set), a bitonic network over the next power of two >= max(n, 256) values (+inf past
 *     n) held in registers, exchanged by lane shuffles and, between waves, through that many doubles of dynamic LDS (64 KiB
 *     at n = 8192).  Equal values are never exchanged; -0.0 and +0.0 compare equal and no output depends on their order.
 *   No atomics: two runs give the same bits, and a direction's w and ks do not depend on the other directions of the call.
 *   ws: mmvae_swd_ws_doubles(n_x, n_y, F, L) = L (n_x + n_y) doubles (the projections, sorted in place; never returned).
 *   1 <= n_x, n_y <= MMVAE_SWD_MAX_ROWS, 1 <= F <= MMVAE_SWD_MAX_F, 1 <= L <= MMVAE_SWD_MAX_DIRECTIONS (axis mode: L == F);
 *   anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.  The rows must be finite (the caller checks).  The helper
 *   is a host function (0 outside the limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_SWD_MAX_ROWS 8192          /* per set */
#define MMVAE_SWD_MAX_F 16384            /* 3 x 64 x 64 pixels = 12288 fit */
#define MMVAE_SWD_MAX_DIRECTIONS 1024
size_t mmvae_swd_ws_doubles(long n_x, long n_y, int F, int L);
int mmvae_swd_slices(const float* X, const float* Y, const double* dirs, double* ws, double* w, long long* ks,
                     long n_x, long n_y, int F, int L, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Cross-modal correlation of generations (TorchMMVAE.cross_modal_correlation; csrc/cca.hip): the canonical-correlation
 * score of image-caption models (Shi et al. 2019), the arithmetic of the reference's cca / apply_weights / apply_pc
 * (eval/mnistsvhn_helper.py:26-78, 149-177), in double, no atomics, every sum in a fixed order: two runs give the same bits.
 *   mmvae_f64_gemm_ld: C (M,N) = A' B (trans_b = 0, B (K,N)) or A' B^T (B (N,K)), A' = A (M,K) with column k multiplied by
 *     scale[k] (scale NULL: A itself, the bits of the plain product), row-major doubles with leading dimensions lda >= K,
 *     ldb >= the width of B, ldc >= N: sub-blocks of larger matrices, read and written in place.  The MFMA tile routine of
 *     mmvae_f64_gemm (64 x 64 per workgroup, k in steps of 4 in order, no K-split); only the (M,N) block of C is written.
 *     C must not overlap A or B.  1 <= M, N, K <= MMVAE_FRECHET_MAX_F.
 *   The fit (ops.cca_fit) is composed from mmvae_sym_eig and this product; see DESIGN.md section 7j.
 *   mmvae_cca_score: a (rows,oa), b (rows,ob) fp32 feature rows; mean_a (oa), mean_b (ob), proj_a (oa,k), proj_b (ob,k)
 *     doubles.  Per row r: p = (a_r - mean_a) proj_a, q = (b_r - mean_b) proj_b, rows converted and centred in double on
 *     load, both products on v_mfma_f64_16x16x4_f64 (64 rows and all k columns per workgroup, the features walked in order
 *     in steps of 4); cos[r] = p . q / (max(|p|, 1e-8) max(|q|, 1e-8)) (F.cosine_similarity's clamp), the three sums of a
 *     row over its columns in a fixed order.  p and q are never written.  sum[0] = sum_r cos[r]: thread t of 256 sums the
 *     rows t, t + 256, ... in order, the partials are added in thread order.  1 <= rows <= MMVAE_CCA_MAX_ROWS,
 *     1 <= oa, ob <= MMVAE_FRECHET_MAX_F, 1 <= k <= MMVAE_CCA_MAX_K.
 *   mmvae_sentence_features: ids (B,T) int32, emb (V,E) fp32, weights (V) fp32, pc (E) doubles or NULL, out (B,E) fp32.
 *     One wave per sentence: L = index of the first `eos` + 1, or T without one; f = (sum_{t < L} weights[id_t] emb[id_t])
 *     / L, the products and the sum in double in token order; with pc, f -= pc (pc . f) (per-lane partials in element
 *     order, a shuffle butterfly); one rounding to fp32.  Every id must lie in [0, V) (ops.sentence_features checks before
 *     the call); a token outside adds nothing and nothing outside the tables is read.  1 <= B <= MMVAE_CCA_MAX_ROWS,
 *     1 <= T <= MMVAE_SENTENCE_MAX_T, 1 <= E <= MMVAE_SENTENCE_MAX_E, V >= 1.
 *   Anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_CCA_MAX_K 64
#define MMVAE_CCA_MAX_VIEWS 8
#define MMVAE_CCA_MAX_ROWS 2147483647L
#define MMVAE_SENTENCE_MAX_E 1024
#define MMVAE_SENTENCE_MAX_T 512
int mmvae_f64_gemm_ld(const double* A, int lda, const double* B, int ldb, double* C, int ldc, const double* scale, int M,
                      int N, int K, int trans_b, mmvae_stream_t stream);
int mmvae_cca_score(const float* a, const float* b, const double* mean_a, const double* mean_b, const double* proj_a,
                    const double* proj_b, double* cos, double* sum, long rows, int oa, int ob, int k, mmvae_stream_t stream);
int mmvae_sentence_features(const int* ids, const float* emb, const float* weights, const double* pc, float* out, long B,
                            int T, int E, int V, int eos, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Latent cluster analysis (TorchMMVAE.cluster_latents; csrc/cluster.hip): k-means (Lloyd) with
 * `restarts` independent fits side by side, the statistics of a partition and the silhouette sums.  X (rows, F) fp32 rows,
 * read as double; centres / means (restarts, C, F) doubles; labels (restarts, rows) int32 in [0, C).
 *   mmvae_cluster_assign: d^2[i, c] = sum_f (x_if - mu_cf)^2 by direct differences, f in order.  given = 0: labels[r, i] =
 *     argmin_c d^2 (a tie goes to the lowest c) is WRITTEN and d2[r, i] = its d^2; given = 1: labels is READ and d2[r, i] =
 *     d^2[i, labels[r, i]] (+inf for a label outside [0, C)).
 *   mmvae_cluster_means: counts[r, c] = n_c; means[r, c, :] = (sum of the rows of cluster c, in index order) / n_c; the
 *     entries of a cluster without rows are left as they are.
 *   mmvae_cluster_spread: from labels and d2 (restarts, rows): counts, within[r, c] = sum_{i in c} d2[r, i], wdist[r, c] =
 *     sum_{i in c} sqrt(d2[r, i]), rows in index order; inertia[r] = sum_c within[r, c], c in order.
 *   mmvae_cluster_lloyd: enqueues the iterations it0 .. it0 + n_iter - 1 (numbered from 1; it0 + n_iter - 1 <= max_iter <=
 *     MMVAE_CLUSTER_MAX_ITER) for all restarts: two launches per iteration and no host synchronisation.  Iteration t:
 *     assignment (labels in place); a restart whose labels all equal the previous iteration's (t > 1) has converged: its
 *     state is written and its centres stay; otherwise the centres become the means (a cluster without rows keeps its
 *     centre and counts the update).  Workgroups of finished restarts return at once.  ws: int32,
 *     mmvae_cluster_lloyd_ws_ints(rows, restarts) = restarts x (4 + ceil(rows / 64) + MMVAE_CLUSTER_MAX_K), ZEROED by the
 *     caller before iteration 1 and carried between calls: (restarts, 4) = (finished, n_iter, converged, unused), then the
 *     blocks' change records (restarts, ceil(rows / 64)), then (restarts, MMVAE_CLUSTER_MAX_K): per cluster the number of
 *     updates it had no rows at (their sum is the restart's `empty`).  labels needs no initial value.  A restart not
 *     finished after max_iter iterations has n_iter = max_iter, converged = 0 (the caller's to write) and needs one more
 *     mmvae_cluster_assign for its labels.
 *   mmvae_cluster_sil_sums: S (rows, C) doubles, S[i, c] = sum_{j in c, j != i} sqrt(max(0, (n2_i + n2_j) - 2 x_i . x_j)),
 *     n2 from mmvae_manifold_sqnorms, the product on the fp64 pair-tile walker of csrc/pair_tile.hpp.  list (padded) int32:
 *     the row numbers sorted by cluster, every cluster's run padded with -1 to a multiple of 64 (padded = 64 x the tiles of
 *     all runs; entries outside [0, rows) count as -1); table (chunks, 3) int32 = (cluster, first tile, tile past the last)
 *     of each chunk, a cluster's chunks consecutive and in order; first (C + 1) int32: cluster c owns the chunks
 *     [first[c], first[c + 1]) (none: its column of S is 0).  Tile numbers are clamped to the list.  One workgroup per
 *     (chunk, row tile) writes one partial per row, ws (chunks, rows) doubles = mmvae_cluster_sil_ws_doubles(rows, chunks);
 *     a merge adds a cluster's chunks in order.  mmvae_cluster_sil_tiles_per_chunk(rows, column tiles, chunks): the column
 *     tiles a chunk holds at the most (chunks 0: the default plan of mmvae_manifold_chunks; a positive value asks for
 *     that many chunks of the whole list).
 *   1 <= rows <= MMVAE_MANIFOLD_MAX_ROWS, 1 <= F <= MMVAE_FRECHET_MAX_F, 1 <= C <= MMVAE_CLUSTER_MAX_K, 1 <= restarts <=
 *   MMVAE_CLUSTER_MAX_INIT; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.  The size helpers are host
 *   functions (0 outside the limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_CLUSTER_MAX_K 64
#define MMVAE_CLUSTER_MAX_INIT 64
#define MMVAE_CLUSTER_MAX_ITER 1000
#define MMVAE_GMM_MAX_D 64              /* csrc/gmm.hip: dimensions of a mixture's rows */
#define MMVAE_GMM_MAX_DRAWS 16777216L  /* draws of one mmvae_gmm_sample call */
size_t mmvae_cluster_lloyd_ws_ints(long rows, int restarts);
int mmvae_cluster_sil_tiles_per_chunk(long rows, int col_tiles, int chunks);
size_t mmvae_cluster_sil_ws_doubles(long rows, int chunks);
int mmvae_cluster_assign(const float* X, const double* centres, int* labels, double* d2, long rows, int F, int C,
                         int restarts, int given, mmvae_stream_t stream);
int mmvae_cluster_means(const float* X, const int* labels, double* means, int* counts, long rows, int F, int C, int restarts,
                        mmvae_stream_t stream);
int mmvae_cluster_spread(const int* labels, const double* d2, int* counts, double* within, double* wdist, double* inertia,
                         long rows, int C, int restarts, mmvae_stream_t stream);
int mmvae_cluster_lloyd(const float* X, double* centres, int* labels, int* ws, long rows, int F, int C, int restarts, int it0,
                        int n_iter, int max_iter, mmvae_stream_t stream);
int mmvae_cluster_sil_sums(const float* X, const double* n2, const int* list, const int* table, const int* first, double* ws,
                           double* S, long rows, int F, int C, long padded, int chunks, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Image reconstruction quality (EvaluationMixin.reconstruction_quality; csrc/image_quality.hip): per pair
 * of images x, y (N, C, H, W) fp32, contiguous, read as double: the errors, PSNR, SSIM (Wang et al. 2004) and multi-scale values.
 *   mmvae_image_quality: out (N, 5 + scales) doubles, row n = (mse, mae, psnr, ssim, ms_ssim, level_1 .. level_scales):
 *     mse / mae = mean of (x - y)^2 / |x - y| over C H W; psnr = 10 log10(data_range^2 / mse), +inf at mse = 0.
 *     Per plane and valid window position (no padding; (H - win + 1) (W - win + 1) of them), with the 2-D weights
 *     window[i] window[j] (`window`: win HOST doubles that sum to 1): mu_x, mu_y the weighted means,
 *     var_x = cov_scale (sum w x^2 - mu_x^2), var_y alike, cov = cov_scale (sum w x y - mu_x mu_y);
 *     l = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1), cs = (2 cov + c2) / (var_x + var_y + c2).  A plane's ssim / cs / l are the
 *     means of l cs / cs / l over its positions, an image's the means of its C planes'.  ssim is level 1's.
 *     Level s + 1 is the 2 x 2 average pooling of level s (in double, on chip, of both images).  level_s = the image's cs of
 *     level s for s < scales and its l for s = scales; ms_ssim = prod_s max(level_s, 0)^ms_weights[s] (`ms_weights`: scales HOST
 *     doubles; scales = 1: ms_ssim = max(ssim, 0), ms_weights is not read).
 *     One launch, one workgroup per image; nothing but `out` is written, no atomics, every sum in a fixed order: a row's bits
 *     do not depend on the other rows of the call.
 *   mmvae_image_quality_max_scales(H, W, win): the deepest `scales` the plane allows (a level that is pooled needs even sides,
 *     every level sides >= win; at most MMVAE_IQ_MAX_SCALES), 0 for a plane or window outside the limits.
 *   mmvae_image_quality_lds_bytes(H, W, win): the LDS of one workgroup (0 outside the limits).  Both are host functions.
 *   win odd in MMVAE_IQ_MIN_WIN .. MMVAE_IQ_MAX_WIN, win <= H, W <= MMVAE_IQ_MAX_SIDE, 1 <= C <= MMVAE_IQ_MAX_CHANNELS,
 *   1 <= scales <= max_scales, 1 <= N <= MMVAE_IQ_MAX_ROWS; anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_IQ_MIN_WIN 3
#define MMVAE_IQ_MAX_WIN 11
#define MMVAE_IQ_MAX_SIDE 64
#define MMVAE_IQ_MAX_CHANNELS 4
#define MMVAE_IQ_MAX_SCALES 4
#define MMVAE_IQ_MAX_ROWS 2147483647L
int mmvae_image_quality_max_scales(int H, int W, int win);
size_t mmvae_image_quality_lds_bytes(int H, int W, int win);
int mmvae_image_quality(const float* x, const float* y, double* out, long N, int C, int H, int W, int win, const double* window,
                        double data_range, double c1, double c2, double cov_scale, int scales, const double* ms_weights,
                        mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Text generation quality (EvaluationMixin.text_quality; csrc/text_quality.hip): per pair of a hypothesis
 * and a reference token sequence the counts behind CER / WER, BLEU, ROUGE-L and exact match, and the reference's negative
 * log-likelihood under the decoder's logits.  One launch, one wave per pair; a pair's outputs depend on nothing but the pair.
 *   mmvae_text_quality: the hypothesis is `logits` (N, Th, V) fp32, or, with logits NULL, `hyp_ids` (N, Th) int32; the
 *     reference `ref_ids` (N, Tr) int32 with `ref_lengths` (N,); `hyp_lengths` (N,) or NULL (every hypothesis Th long).
 *     eos, trim, sep: token ids, negative for none.
 *     1. logits: pred[n, t] = the first maximum over V (the rule of mmvae_text_decode_score; an all-equal row gives 0) is the
 *        hypothesis; nll[n] = sum_{t < S} (lse_t - x_t[ref_t]), S = min(clamp(ref_length, 0, Tr), Th) = nll_steps[n], in double
 *        from the fp32 values: lse_t = m_t + log sum_v exp(x_v - m_t), m_t the row's maximum, v rising; the steps t = l, l + 64,
 *        .. are summed in that order per l < 64, the 64 sums by butterfly (xor 32, 16, .. 1).  Reference ids read here are
 *        clamped into [0, V): a caller checks them.  Finite logits.
 *     2. both sides: length = clamp(given length, 0, T); with eos the sequence ends before the first eos; with trim the
 *        trailing tokens equal to trim are then dropped: h (Lh tokens) and r (Lr).
 *     3. token_out (N, 13) = hyp_len Lh, ref_len Lr, same, edit, lcs, match[4], total[4]:
 *        same = #{t < min(Lh, Lr): h_t == r_t}; edit = Levenshtein distance (unit costs); lcs = longest common subsequence;
 *        for n = 1 .. max_order: total_n = max(Lh - n + 1, 0), match_n = sum over the distinct n-grams g of h of
 *        min(count_h(g), count_r(g)); the columns n > max_order are 0.
 *     4. sep >= 0: word_out (N, 12) = hyp_len, ref_len, edit, lcs, match[4], total[4] of the word sequences: words are the
 *        maximal runs of tokens != sep inside h and r, equal iff they have the same tokens (compared token by token).
 *        sep < 0: word_out NULL.
 *     pred, nll, nll_steps are written for logits only (NULL otherwise).  Ids are non-negative.
 *   mmvae_text_quality_lds_bytes(Th, Tr): the LDS of one workgroup (0 outside the limits); a host function.
 *   1 <= Th, Tr <= MMVAE_TQ_MAX_STEPS, 2 <= V <= MMVAE_TQ_MAX_VOCAB, 1 <= max_order <= MMVAE_TQ_MAX_ORDER,
 *   1 <= N <= MMVAE_TQ_MAX_ROWS = 2^26 - 1 (one launch of N workgroups of 64 threads: the grid stays below 2^32 threads; a
 *   caller with more pairs calls again); anything else returns MMVAE_ERR_UNSUPPORTED and writes nothing.
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_TQ_MAX_STEPS 256
#define MMVAE_TQ_MAX_VOCAB 256
#define MMVAE_TQ_MAX_ORDER 4
#define MMVAE_TQ_MAX_ROWS 67108863L
size_t mmvae_text_quality_lds_bytes(int Th, int Tr);
int mmvae_text_quality(const float* logits, const int* hyp_ids, const int* ref_ids, const int* ref_lengths,
                       const int* hyp_lengths, int* pred, int* token_out, int* word_out, double* nll, int* nll_steps, long N,
                       int Th, int Tr, int V, int eos, int trim, int sep, int max_order, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Cross-modal retrieval of latents (EvaluationMixin.cross_modal_retrieval; csrc/retrieval.hip): are the
 * sets aligned row by row?  loc (S, N, D) fp32, scale (S, N, D) fp32 or NULL (l2, cosine); pairs (P, 2) int32 = (query set,
 * gallery set) in [0, S), the two different; match (N,) int32 or NULL for the identity: match[i] = the gallery row that is
 * query row i's partner, -1 (or anything outside [0, N)) = no partner.  Distance of a query row q and a gallery row g, in
 * double from the fp32 values converted on load, by direct differences, the dimensions summed in order with fma:
 *   MMVAE_RETRIEVAL_L2      sum (mq - mg)^2
 *   MMVAE_RETRIEVAL_COSINE  1 - sum mq mg / sqrt(sum mq^2 . sum mg^2); 1 when either norm is 0
 *   MMVAE_RETRIEVAL_W2      sum (mq - mg)^2 + (sq - sg)^2          (squared 2-Wasserstein distance of diagonal Gaussians)
 *   MMVAE_RETRIEVAL_SKL     sum 1/2 [(sq^2 + D^2) / sg^2 + (sg^2 + D^2) / sq^2] - 1, D = mq - mg     (KL(q || g) + KL(g || q))
 * A pair's distance is a function of its two rows alone (one accumulator type serves the matched pair and every other pair;
 * no dependence on tile, chunk or launch shape), so the comparisons below are exact with respect to these distances.
 * Per (pair p, query row i), with m = match[i]:
 *   d_match (P, N) doubles   d(i, m); NaN without a partner
 *   less, equal (P, N) int32 #{j != m : d(i, j) < d_match}, #{j != m : d(i, j) == d_match}; -1, -1 without a partner
 *   nn_d, nn_idx (P, N, keep) doubles / int32, keep > 0: the keep nearest gallery rows (the partner among them), ordered by
 *     (distance, index); (+inf, -1) in the slots beyond N
 * The N x N distances are never written; no atomics.  A workgroup owns 64 query rows and a chunk of gallery rows staged 32 at a
 * time in LDS as doubles (mean; w2: scale; skl: variance and its reciprocal -- one divide per staged element); grid (chunks,
 * row tiles, P): one launch serves all pairs, and with more than one chunk a second merges the chunks' partials in chunk order
 * (integer sums; the keep smallest by (distance, index)).  The outputs are the same bits under any chunks, for two runs, and
 * for a pair alone or beside other pairs.
 *   chunks: 0 = the default plan, mmvae_retrieval_chunks(N, P) = min(ceil(1024 / (ceil(N / 64) P)), ceil(tiles / 8)), tiles =
 *     ceil(N / 32); a positive value asks for that many (at most one per tile); chunks that would be empty are not launched.
 *   ws: mmvae_retrieval_ws_bytes(N, P, keep, chunks) bytes, a multiple of 8 (0 for one chunk: ws may be NULL), 8-byte
 *     aligned = (chunk, P, N, keep) doubles | the same int32 | less (chunk, P, N) | equal.
 *   1 <= N <= MMVAE_RETRIEVAL_MAX_ROWS, 1 <= D <= MMVAE_RETRIEVAL_MAX_DIM, 2 <= S <= MMVAE_RETRIEVAL_MAX_SETS, 1 <= P <=
 *   MMVAE_RETRIEVAL_MAX_PAIRS, 0 <= keep <= MMVAE_RETRIEVAL_MAX_KEEP, chunks >= 0; anything else returns
 *   MMVAE_ERR_UNSUPPORTED and writes nothing; w2 / skl without scale is MMVAE_ERR_ARG.  Finite loc, scale > 0 and the entries
 *   of pairs are the caller's to check (a pair outside [0, S) is skipped).  The two helpers are host functions (0 outside the
 *   limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_RETRIEVAL_MAX_ROWS 16384
#define MMVAE_RETRIEVAL_MAX_DIM 256
#define MMVAE_RETRIEVAL_MAX_SETS 16
#define MMVAE_RETRIEVAL_MAX_PAIRS 240
#define MMVAE_RETRIEVAL_MAX_KEEP 16
#define MMVAE_RETRIEVAL_L2 0
#define MMVAE_RETRIEVAL_COSINE 1
#define MMVAE_RETRIEVAL_W2 2
#define MMVAE_RETRIEVAL_SKL 3
int mmvae_retrieval_chunks(long N, int P);
size_t mmvae_retrieval_ws_bytes(long N, int P, int keep, int chunks);
int mmvae_retrieval_ranks(const float* loc, const float* scale, const int* pairs, const int* match, void* ws, double* d_match,
                          int* less, int* equal, double* nn_d, int* nn_idx, long N, int D, int S, int P, int metric, int keep,
                          int chunks, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Latent density estimation (EvaluationMixin.fit_latent_density / sample_latent_density; csrc/gmm.hip):
 * EM for a mixture of C Gaussians on the rows of X (rows, D) fp32, read as double, `restarts` independent fits side by side,
 * covariances MMVAE_GMM_FULL or MMVAE_GMM_DIAG, everything in double with scikit-learn's GaussianMixture arithmetic.
 * Parameters per restart: weights (R, C), means (R, C, D), cov / chol / prec (R, C, D, D) (diag: (R, C, D)) = the covariance,
 * its lower Cholesky factor L (diag: its square root) and the precision factor P = L^-T, upper triangular (diag: 1 / sqrt),
 * logdet (R, C) = sum_d log P[d, d]; resp (R, rows, C).
 *   E-step   log p_ik = log w_k - (D log 2 pi + |(x_i - mu_k)^T P_k|^2) / 2 + logdet_k; norm_i = logsumexp_k log p_ik (the largest
 *            taken out); resp_ik = exp(log p_ik - norm_i); the lower bound is the mean of norm_i.
 *   M-step   n_k = sum_i r_ik + 10 DBL_EPSILON; mu_k = sum_i r_ik x_i / n_k; full: S_k = sum_i r_ik (x_i - mu_k)(x_i - mu_k)^T
 *            / n_k + reg_covar I; diag: sum_i r_ik x_i^2 / n_k - mu_k^2 + reg_covar; w_k = (n_k / rows) / sum_k (n_k / rows);
 *            then L_k, P_k, logdet_k.  Sums over rows: 64-row blocks (1024-row chunks for the covariances) summed in row order
 *            and merged in block order.  No atomics.
 *   mmvae_gmm_em: enqueues the iterations it0 .. it0 + n_iter - 1 (numbered from 1; it0 + n_iter - 1 <= max_iter <=
 *     MMVAE_CLUSTER_MAX_ITER) for all restarts, three launches per iteration and no host synchronisation; with it0 = 1 the
 *     start comes first: resp = the one-hot of init (R, rows) int32 (an id outside [0, C) leaves the row out) and an M-step.
 *     Iteration t: an E-step with the current parameters, an M-step; lb_t = that E-step's bound; |lb_t - lb_{t-1}| < tol
 *     (lb_0 = -inf): the restart has converged, with the parameters of this M-step.  A Cholesky pivot that is not positive
 *     and finite makes the restart degenerate.  Workgroups of a converged or degenerate restart return at once.
 *     ws: mmvae_gmm_ws_doubles(rows, D, C, restarts, diag) doubles, ZEROED by the caller before iteration 1 and carried
 *     between calls.  It begins with (restarts, 4) = (lb_t, n_iter = t of the last iteration run, converged, stamp: nonzero
 *     once converged), then (restarts, MMVAE_CLUSTER_MAX_K): nonzero where a component's factorisation failed.  Neither
 *     resp nor a density of the final parameters is left behind: mmvae_gmm_score gives them.
 *   mmvae_gmm_score: the E-step's code on any rows under given parameters: logdens (R, rows) = norm_i; resp (R, rows, C) and
 *     labels (R, rows) int32 = the first largest log p_ik, either may be NULL.
 *   mmvae_gmm_sample: n draws from ONE mixture (weights (C), means (C, D), chol): draw i takes the first component k with
 *     u[i] < w_0 + .. + w_k (summed in order, the last component takes the rest) and z = mu_k + L_k eps[i] (diag: mu_k +
 *     sqrt(S_k) eps[i]) in double, rounded to fp32 once; u (n) doubles in [0, 1), eps (n, D) fp32; z (n, D) fp32, comp (n) int32.
 *   1 <= rows <= MMVAE_MANIFOLD_MAX_ROWS, 1 <= D <= MMVAE_GMM_MAX_D, 1 <= C <= MMVAE_CLUSTER_MAX_K, 1 <= restarts <=
 *   MMVAE_CLUSTER_MAX_INIT, reg_covar >= 0, tol >= 0, 1 <= n <= MMVAE_GMM_MAX_DRAWS; anything else returns
 *   MMVAE_ERR_UNSUPPORTED and writes nothing.  The size helper is a host function (0 outside the limits).
 * ---------------------------------------------------------------------------------------------- */
#define MMVAE_GMM_FULL 0
#define MMVAE_GMM_DIAG 1
size_t mmvae_gmm_ws_doubles(long rows, int D, int C, int restarts, int diag);
int mmvae_gmm_em(const float* X, const int* init, double* weights, double* means, double* cov, double* chol, double* prec,
                 double* logdet, double* resp, double* ws, long rows, int D, int C, int restarts, int diag, double reg_covar,
                 double tol, int it0, int n_iter, int max_iter, mmvae_stream_t stream);
int mmvae_gmm_score(const float* X, const double* weights, const double* means, const double* prec, const double* logdet,
                    double* logdens, double* resp, int* labels, long rows, int D, int C, int restarts, int diag,
                    mmvae_stream_t stream);
int mmvae_gmm_sample(const double* weights, const double* means, const double* chol, const double* u, const float* eps,
                     float* z, int* comp, long n, int D, int C, int diag, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Text towers (Enc_TxtTransformer / Dec_TxtTransformer, models/encoders.py:790-837, decoders.py:668-723)
 * ---------------------------------------------------------------------------------------------- */
/* Embedding(one-hot.long()) + PositionalEncoding quirk (models/nn_modules.py:430-438, encoders.py:833-835).
 *   onehot (B,T,V) 0/1 floats, emb (V,2) [only rows 0/1 are read], pe (>= max(B,T), 2) = the module's
 *   sin/cos buffer (host-computed once), x (T*B, 2V) = the (nframes,bs,-1) view.
 *   mode 0 (B != T, B != 1): x[t,b,v,e] = emb[oh[b,t,v],e] + pe[b,e]
 *   mode 1 (B == T or B == 1): memory (B,T,2V) with pe[t] (pe[0] if B == 1), relabelled as (T,B,2V).
 *   B0 (round 5): onehot has B0 rows, B = R * B0 output rows, row b reads onehot row and pe row b % B0 (mode 0 only
 *   when B0 < B): R passes over the same batch as one call (POE's per-subset passes, models/mmvae_models.py:159-187). */
int mmvae_embed_pe_fwd(const float* onehot, const float* emb, const float* pe, float* x, int B, int T, int V,
                       int mode, int B0, const mmvae_dropout_t* drop, mmvae_stream_t stream);
int mmvae_embed_pe_bwd(const float* onehot, const float* dx, float* demb, float* ws, int B, int T, int V, int mode,
                       int B0, int accumulate, const mmvae_dropout_t* drop, mmvae_stream_t stream);
size_t mmvae_embed_ws_floats(int B, int T, int V);

/* ---- One Transformer layer of the text towers per launch (csrc/txtlayer.hip) --------------------------------
 * torch.nn.TransformerEncoderLayer / TransformerDecoderLayer (post-norm, gelu, dropout p) as the reference builds
 * them: models/encoders.py:806-812 (Enc_TxtTransformer, d = 2V = 54, ff 128, 2 heads) and models/decoders.py:686-692
 * (Dec_TxtTransformer, d = n_latents, memory length 1).  One workgroup per sequence, L <= 32 tokens; activations are
 * (L, N, D) time-major like the rest of the text path.  Shapes outside mmvae_txt_layer_supported() use the op-by-op
 * entry points below (same arithmetic, same dropout masks).
 *   fwd writes y and the tensors backward needs; bwd runs the whole data-gradient chain and leaves the output
 *   gradient of every GEMM in HBM (d_*), from which the weight gradients are mmvae_linear_bwd_weight calls over the
 *   (L*N)-row tensors:  in_proj (d_qkv, x) | out_proj (d_a, ao) | linear1 (d_h1, x1 or x2) | linear2 (d_f, g)
 *   decoder: cross out_proj (d_ca, vb) | cross value projection (d_v (N,D), mem).
 *   lnws (N, n_norms, 2, D): per-sequence partials of the LayerNorm gamma / beta gradients (norm order 1, [2,] last). */
typedef struct {
  const float *in_w, *in_b;     /* self-attention in_proj (3D, D), (3D) */
  const float *out_w, *out_b;   /* self-attention out_proj (D, D), (D) */
  const float *l1_w, *l1_b;     /* linear1 (FF, D), (FF) */
  const float *l2_w, *l2_b;     /* linear2 (D, FF), (D) */
  const float *n1_g, *n1_b, *n2_g, *n2_b, *n3_g, *n3_b; /* LayerNorm weight / bias; n3 decoder only */
  const float *x_in_w, *x_in_b; /* decoder: VALUE rows of the cross-attention in_proj (D, D), (D) */
  const float *x_out_w, *x_out_b; /* decoder: cross-attention out_proj */
} mmvae_txt_layer_w_t;
typedef struct {
  float *qkv;                   /* (L,N,3D) */
  float *probs;                 /* (N,H,L,L) normalised attention weights before dropout, or NULL */
  float *ao;                    /* (L,N,D) attention output (input of out_proj) */
  float *xhat1, *rstd1, *x1;    /* LayerNorm1: (L,N,D), (L,N), output (L,N,D) */
  float *vproj, *vb;            /* decoder: value projection (N,D); its dropout-masked broadcast (L,N,D) */
  float *xhat2, *rstd2, *x2;    /* decoder LayerNorm2 */
  float *h1, *g;                /* linear1 output (L,N,FF); dropout(gelu(h1)) (L,N,FF) */
  float *xhatf, *rstdf;         /* last LayerNorm */
} mmvae_txt_layer_saved_t;
typedef struct {
  float *d_f, *d_h1, *d_ca, *d_v, *d_a, *d_qkv, *lnws;
} mmvae_txt_layer_grads_t;
typedef struct {
  mmvae_dropout_t attn, drop1, xattn, drop2, ffn, drop3; /* encoder: attn, drop1, ffn, drop2 */
} mmvae_txt_layer_drop_t;
int mmvae_txt_layer_supported(int L, int D, int FF, int NH, int dec);
/* Round 4: two kernel families serve these entry points -- one workgroup per sequence (csrc/txtlayer.hip) and one WAVE
 * per sequence with the activations chained through registers (csrc/txtwave.hip; forward always, backward from 384
 * sequences).  Same arithmetic, saved tensors and masks; this sets the choice (-1 keeps a value): forward on the wave
 * kernels, backward on them from bwd_min_n sequences (d > 32 layers) / bwd_min_n_dec (d <= 32 decoder layers).
 * Defaults from MMVAE_TXT_WAVE / MMVAE_TXT_WAVE_BWD_MIN_N[_DEC]. */
int mmvae_txt_layer_plan(int fwd_wave, int bwd_min_n, int bwd_min_n_dec);
size_t mmvae_txt_layer_lnws_floats(int N, int D, int dec);
/* time_mean != 0: y / dy are (N, D), the mean of the layer output over the L frames and its gradient -- the pooling
 * `x.mean(0)` that follows the last encoder layer (models/encoders.py:552), folded into the layer's launch */
/* head_w (HN, D), head_b (HN) non-NULL (needs time_mean): additionally heads (N, HN) = y head_w^T + head_b, the
 * packed posterior heads on the pooled feature (VaeComponent.process_output, models/encoders.py:49-54); their
 * backward is an ordinary mmvae_linear_bwd on (heads gradient, y) */
int mmvae_txt_layer_fwd(const float* x, const uint8_t* valid, const float* mem, float* y,
                        const mmvae_txt_layer_w_t* w, const mmvae_txt_layer_saved_t* saved,
                        const mmvae_txt_layer_drop_t* drop, int L, int N, int D, int FF, int NH, int dec,
                        int time_mean, const float* head_w, const float* head_b, float* heads, int HN,
                        mmvae_stream_t stream);
int mmvae_txt_layer_bwd(const float* dy, const uint8_t* valid, float* dx, float* dmem,
                        const mmvae_txt_layer_w_t* w, const mmvae_txt_layer_saved_t* saved,
                        const mmvae_txt_layer_grads_t* grads, const mmvae_txt_layer_drop_t* drop, int L, int N, int D,
                        int FF, int NH, int dec, int time_mean, mmvae_stream_t stream);

/* Input expansion on the device (the step in front of the path): bit-identical to the reference's
 * host-side `torch.tensor(uint8) / 255` (models/datasets.py:251-254) and `one_hot_encode` + `lengths_to_mask`
 * (utils.py:414-421, :239; models/datasets.py:272-281).  tokens (B,T) int32, -1 = character outside the alphabet (zero
 * row); lengths (B); onehot (B,T,V) fp32; mask (B,T) bytes, may be NULL. */
int mmvae_expand_image_u8(const uint8_t* src, float* dst, long n, mmvae_stream_t stream);
int mmvae_expand_text_tokens(const int32_t* tokens, const int32_t* lengths, float* onehot, uint8_t* mask, int B, int T,
                             int V, mmvae_stream_t stream);
/* The host-to-device transfer of the NEXT batch as a node inside the captured step: ring_dev = device array of n_ring
 * pinned (device-visible, 16-byte aligned) host batches of `bytes` bytes; ctr_dev = two device words {count, ticket}
 * (zeroed once); the launch copies bytes [offset, offset + bytes) of ring[count % n_ring] into the same range of
 * `staging` and, when `advance` is set, advances count itself (a batch may be pulled in several parts: the last one
 * advances). */
int mmvae_input_ring_pull(const void* const* ring_dev, int n_ring, unsigned* ctr_dev, void* staging, size_t offset,
                          size_t bytes, int advance, mmvae_stream_t stream);

/* The input step as a native pipe: a packed pinned host batch (every tensor a 16-byte aligned slice of one buffer) is
 * copied with ONE H2D transfer on the pipe's own copy stream into `staging` (device, `bytes` long, owned by the
 * caller), under the step that is running; mmvae_input_pipe_commit then, on `stream`: waits for that copy, expands
 * every modality into the step's static inputs (the two functions above), marks the staging buffer consumed and --
 * `next_host_packed` != NULL -- starts the copy of the following batch behind that.  One call per step.
 * Replaces, on the caller side of the path, the reference's per-step DataLoader -> device transfer of fp32 images and
 * one-hot text (models/dataloader.py:120-126; tensors built by models/datasets.py:251-254, :272-281). */
#define MMVAE_INPUT_MAX_MODS 8
#define MMVAE_INPUT_IMAGE_U8 0
#define MMVAE_INPUT_TEXT_TOKENS 1
typedef struct mmvae_input_pipe mmvae_input_pipe_t;
typedef struct {
  int kind;         /* MMVAE_INPUT_IMAGE_U8 | MMVAE_INPUT_TEXT_TOKENS */
  size_t src_off;   /* byte offset in the packed batch: uint8 pixels | (B,T) int32 tokens */
  size_t len_off;   /* text: byte offset of the (B) int32 lengths */
  float* dst;       /* fp32 image (n values) | one-hot (B,T,V) */
  uint8_t* mask;    /* text: (B,T) bytes or NULL */
  long n;           /* image: number of pixel values */
  int B, T, V;      /* text */
} mmvae_input_mod_t;
int mmvae_input_pipe_create(mmvae_input_pipe_t** out, void* staging, size_t bytes);
int mmvae_input_pipe_destroy(mmvae_input_pipe_t* pipe);
int mmvae_input_pipe_prefetch(mmvae_input_pipe_t* pipe, const void* host_packed);
int mmvae_input_pipe_commit(mmvae_input_pipe_t* pipe, const mmvae_input_mod_t* mods, int n_mods,
                            const void* next_host_packed, mmvae_stream_t stream);

/* y[t,b,:] = dropout(x[t,b,:] + pe[t,:]) -- Enc_Transformer / Dec_Transformer positional encoding
 * (models/encoders.py:721-723, models/decoders.py:607-608; PositionalEncoding try-branch nn_modules.py:430-438).
 * x may be NULL (time queries PE(zeros)).  Backward: mmvae_dropout_act_bwd with MMVAE_ACT_NONE. */
int mmvae_add_pe_dropout_fwd(const float* x, const float* pe, float* y, int T, int B, int D,
                             const mmvae_dropout_t* drop, mmvae_stream_t stream);

/* Scaled-dot-product attention with key padding mask for L, S <= 128 and head_dim hd <= 32 (nn.MultiheadAttention core;
 * MMVAE_ERR_UNSUPPORTED past either limit, nothing written).
 *   q (L*N, ldq) rows r = l*N+n, head h at columns [h*hd,(h+1)*hd); k, v (S*N, ld) likewise.
 *   kpm (N,S) bytes, 1 = ignore key (may be NULL); with mask_is_valid != 0 the bytes are the batch's validity
 *   mask instead (1 = real token).  out (L*N, E=H*hd).  probs (N,H,L,S) saved for bwd: the normalised weights before
 *   dropout, a weight that the dropout removed stored NEGATED (sign bit = the mask: mmvae_attn_bwd hashes nothing). */
int mmvae_attn_fwd(const float* q, const float* k, const float* v, const uint8_t* kpm, float* out, float* probs,
                   int L, int S, int N, int H, int hd, long ldq, long ldk, long ldv, int mask_is_valid,
                   const mmvae_dropout_t* drop, mmvae_stream_t stream);
int mmvae_attn_bwd(const float* q, const float* k, const float* v, const float* probs, const float* dout,
                   float* dq, float* dk, float* dv, int L, int S, int N, int H, int hd, long ldq, long ldk,
                   long ldv, const mmvae_dropout_t* drop, mmvae_stream_t stream);
/* runtime switch between the two MFMA backward kernels of mmvae_attn_bwd for 32 < L, S <= 128: 0 (default) = the LDS-tile form,
 * 1 = the register form (csrc/text.hip: attn_t_bwd_kernel, needs 16-byte aligned head slices; measured level in the step);
 * returns the previous setting.  MMVAE_ATTN_T_BWD=1 in the environment starts with 1.  (nn.MultiheadAttention backward: reference models/encoders.py:706-716) */
int mmvae_attn_t_bwd_set(int on);
/* Which kernel instantiation of csrc/text.hip serves a call: one value per instantiation, returned by mmvae_attn_path and
 * switched on by mmvae_attn_fwd / mmvae_attn_bwd themselves (the query IS the dispatch).  ROW = thread per query row / key
 * column, <threads, padded head_dim>; MFMA = the LDS-tile MFMA kernels; T = the transposed forward / register-form backward.
 *   hd <= 16 and (L > 32 or S > 32):  T_FWD if hd % 4 == 0, ldq, ldk, ldv % 4 == 0 and aligned16, else MFMA_FWD;
 *                                     T_BWD under the same condition AND mmvae_attn_t_bwd_set(1), else MFMA_BWD;
 *   otherwise ROW: 64 threads up to L, S <= 64, else 128; padded head_dim 16 up to hd <= 16, else 32.
 * (so ROW_*_128_16 is built but no supported shape reaches it.) */
enum {
  MMVAE_ATTN_ROW_FWD_64_16 = 16,
  MMVAE_ATTN_ROW_FWD_64_32,
  MMVAE_ATTN_ROW_FWD_128_16,
  MMVAE_ATTN_ROW_FWD_128_32,
  MMVAE_ATTN_MFMA_FWD,
  MMVAE_ATTN_T_FWD,
  MMVAE_ATTN_ROW_BWD_64_16,
  MMVAE_ATTN_ROW_BWD_64_32,
  MMVAE_ATTN_ROW_BWD_128_16,
  MMVAE_ATTN_ROW_BWD_128_32,
  MMVAE_ATTN_MFMA_BWD,
  MMVAE_ATTN_T_BWD
};
/* Pure query (launches nothing, needs no GPU).  bwd: 0 = mmvae_attn_fwd, 1 = mmvae_attn_bwd.  aligned16 != 0: every pointer
 * the float4 paths touch is 16-byte aligned (forward: q, k, v; backward: q, k, v, dout, dq, dk, dv).  Returns one of the
 * values above, MMVAE_ERR_UNSUPPORTED past L, S <= 128 / hd <= 32, MMVAE_ERR_ARG for a non-positive size. */
int mmvae_attn_path(int bwd, int L, int S, int hd, long ldq, long ldk, long ldv, int aligned16);

/* y = LayerNorm(x + r) * gamma + beta (eps 1e-5); r may be NULL, same-shape (r_rows = 0) or broadcast over time
 * (r_rows = N: row index = row % N).  xhat (rows,d) and rstd (rows) are saved for the backward.
 * With dropout: y = LN(dropout(x) + r).
 * bwd: dsum = grad wrt the sum (= grad of r); with dropout dx_drop = dsum * mask is the grad of x;
 * dgamma/dbeta (+)= through ws (mmvae_layernorm_ws_floats). */
int mmvae_layernorm_residual_fwd(const float* x, const float* r, const float* gamma, const float* beta, float* y,
                                 float* xhat, float* rstd, int rows, int d, int r_rows, const mmvae_dropout_t* drop,
                                 mmvae_stream_t stream);
int mmvae_layernorm_residual_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma,
                                 float* dsum, float* dx_drop, float* dgamma, float* dbeta, float* ws, int rows, int d,
                                 int accumulate, const mmvae_dropout_t* drop, mmvae_stream_t stream);
size_t mmvae_layernorm_ws_floats(int rows, int d);

/* mean over the leading (time) axis: x (L,N,d) -> y (N,d)  (encoders.py:836); bwd: dx = dy / L broadcast */
int mmvae_mean_over_time_fwd(const float* x, float* y, int L, int N, int d, mmvae_stream_t stream);
int mmvae_mean_over_time_bwd(const float* dy, float* dx, int L, int N, int d, mmvae_stream_t stream);

/* rows of (L,N,d) summed over time into (N,d): used for the broadcast cross-attention gradient */
int mmvae_sum_over_time(const float* x, float* y, int L, int N, int d, mmvae_stream_t stream);

/* y[r, :] = x[r, :] * m[r]  with rows r = (t,b) of a (T,B,V) tensor written as (B,T,V): the decoder's
 * permute(1,0,2) * mask (decoders.py:722).  in (T*B, V) -> out (B,T,V);  bwd is the inverse scatter. */
int mmvae_permute_mask_fwd(const float* x, const uint8_t* mask, float* y, int T, int B, int V,
                           mmvae_stream_t stream);
int mmvae_permute_mask_bwd(const float* dy, const uint8_t* mask, float* dx, int T, int B, int V,
                           mmvae_stream_t stream);
/* ... the first Tk <= T steps only: out (B,Tk,V); mask stays (B,T).  bwd: dy (B,Tk,V) -> dx (T,B,V), exact zeros from step
 * Tk on.  The reference slices the permuted, masked decoder output to the target's mask length (BaseObjective.recon_loss_fn,
 * models/objectives.py:30-52, behind models/decoders.py:720-722): the two as one launch per direction. */
int mmvae_permute_mask_head_fwd(const float* x, const uint8_t* mask, float* y, int T, int B, int V, int Tk,
                                mmvae_stream_t stream);
int mmvae_permute_mask_head_bwd(const float* dy, const uint8_t* mask, float* dx, int T, int B, int V, int Tk,
                                mmvae_stream_t stream);

/* Standard-normal noise for the reparameterised samples (the reference draws it with torch.distributions rsample:
 * models/mmvae_models.py:363-369).  state = {seed, call counter, ticket} (three uint32 on the device, ticket 0); the
 * launch advances the call counter itself, so a captured graph replays with fresh noise and no host work. */
int mmvae_randn(float* out, long n, uint32_t* state, mmvae_stream_t stream);

/* debug: store the device wall clock (100 MHz ticks) into *slot, in stream order (phase timelines of a graph replay) */
int mmvae_debug_timestamp(long long* slot, mmvae_stream_t stream);
/* debug: one thread spins for `ticks` device wall-clock ticks, then stores {start, end} ticks into slot[0..1] */
int mmvae_debug_spin(long long* slot, long long ticks, mmvae_stream_t stream);

/* ---- Generic convolutions (csrc/conv_generic.hip): any channel counts, K <= 4, stride S, padding P -------------
 * First correct path for Enc_SVHN / Dec_SVHN (models/encoders.py:434-478, models/decoders.py:101-147); plain fp32 FMA.
 * Same conventions as the k4-s2-p1 entry points above: layers emit pre-activations, `in_act` is applied to the
 * input, `ep_mode` to the output (`aux` = the tensor a MUL_* epilogue differentiates through).
 *   Conv2d          w [Cout][Cin][K][K], Hout = (Hin + 2P - K) / S + 1
 *   ConvTranspose2d w [Cin][Cout][K][K], Hout = (Hin - 1) S - 2P + K                                            */
int mmvae_conv2d_generic_fwd(const float* x, const float* w, const float* bias, const float* aux, float* y, int B,
                             int Cin, int Cout, int Hin, int Win, int K, int S, int P, int in_act, int ep_mode,
                             mmvae_stream_t stream);
int mmvae_conv2d_generic_dgrad(const float* dy, const float* w, const float* aux, float* dx, int B, int Cin, int Cout,
                               int Hin, int Win, int K, int S, int P, int ep_mode, mmvae_stream_t stream);
int mmvae_conv2d_generic_wgrad(const float* dy, const float* x, float* dw, float* db, int B, int Cin, int Cout, int Hin,
                               int Win, int K, int S, int P, int x_act, int accumulate, mmvae_stream_t stream);
int mmvae_convT2d_generic_fwd(const float* x, const float* w, const float* bias, const float* aux, float* y, int B,
                              int Cin, int Cout, int Hin, int Win, int K, int S, int P, int in_act, int ep_mode,
                              mmvae_stream_t stream);
int mmvae_convT2d_generic_dgrad(const float* dy, const float* w, const float* aux, float* dx, int B, int Cin, int Cout,
                                int Hin, int Win, int K, int S, int P, int ep_mode, mmvae_stream_t stream);
int mmvae_convT2d_generic_wgrad(const float* dy, const float* x, float* dw, float* db, int B, int Cin, int Cout,
                                int Hin, int Win, int K, int S, int P, int x_act, int accumulate,
                                mmvae_stream_t stream);
/* y = sigmoid(x); dx = dy y (1 - y)   (Dec_MNIST, models/decoders.py:266; backward of MMVAE_EP_SIGMOID outputs) */
int mmvae_sigmoid_fwd(const float* x, float* y, long n, mmvae_stream_t stream);
int mmvae_sigmoid_bwd(const float* dy, const float* y, float* dx, long n, mmvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser + utilities
 * ---------------------------------------------------------------------------------------------- */
/* torch.optim.Adam(amsgrad=True) over one flat buffer (models/trainer.py:79-81); step is 1-based and is
 * read from *step_dev (device int) when step_dev != NULL, so that a captured hipGraph replays with the
 * right bias correction (mmvae_step_inc bumps it on the stream).  With step < 0, step_dev is a zero-initialised,
 * 8-byte aligned 24-byte block {int count, int ticket, double beta1^count, double beta2^count}: the launch is step
 * count + 1 and stores the new count and powers itself when its last workgroup finishes -- no separate launch.  g is multiplied by grad_scale first (1/world_size after a sum all-reduce);
 * zero_grad != 0 clears g. */
int mmvae_adam_amsgrad_flat(float* p, float* g, float* m, float* v, float* vmax, long n, float lr, float beta1,
                            float beta2, float eps, int step, int* step_dev, float grad_scale,
                            int zero_grad, mmvae_stream_t stream);
/* `optimizer: adabelief` (models/trainer.py:82-86: adabelief_pytorch.AdaBelief(lr, eps=1e-16, betas=(0.9, 0.999),
 * weight_decouple=True, rectify=False), weight_decay 0): m = b1 m + (1-b1) g; s = b2 s + (1-b2)(g-m)^2 + eps;
 * p -= lr/bc1 * m / (sqrt(s)/sqrt(bc2) + eps).  The package is not vendored by the reference and absent here: restated
 * from Zhuang et al. 2020 (Algorithm 2) and the package's update order, parity unpinned.  step / step_dev / grad_scale /
 * zero_grad as mmvae_adam_amsgrad_flat. */
int mmvae_adabelief_flat(float* p, float* g, float* m, float* s, long n, float lr, double beta1, double beta2, float eps,
                         int step, int* step_dev, float grad_scale, int zero_grad, mmvae_stream_t stream);
int mmvae_step_inc(int* step_dev, mmvae_stream_t stream);
/* dst[i] (+)= sum_r src[r*stride + i],  i < len */
int mmvae_reduce_rows(const float* src, float* dst, int n_rows, long len, long stride, int accumulate,
                      mmvae_stream_t stream);
int mmvae_fill(float* p, long n, float value, mmvae_stream_t stream);

/* Deferred gradient reduction.  With accumulate == MMVAE_ACC_DEFER the *_wgrad / *_bwd_weight / layernorm /
 * embed backward entry points only leave their split partials in `ws` (which must then be private to that call
 * until the reduction runs); the *_layout queries describe them, and ONE mmvae_reduce_segments launch at the end
 * of backward adds every registered segment into its destination:  dst[i] += sum_r src[r*stride + i]. */
#define MMVAE_ACC_DEFER 2
#define MMVAE_MAX_SEGMENTS 64
typedef struct {
  const float* src[MMVAE_MAX_SEGMENTS];
  float* dst[MMVAE_MAX_SEGMENTS];
  int rows[MMVAE_MAX_SEGMENTS];
  int len[MMVAE_MAX_SEGMENTS];
  int stride[MMVAE_MAX_SEGMENTS];
  int blk0[MMVAE_MAX_SEGMENTS]; /* filled by the library */
  int next[MMVAE_MAX_SEGMENTS]; /* filled by the library: chain of segments sharing one destination */
  int n;
} mmvae_reduce_segments_t;
int mmvae_reduce_segments(const mmvae_reduce_segments_t* table, mmvae_stream_t stream);
/* ... with the ELBO assembly of mmvae_lincomb_rowptrs_fwd (out[k] = sum_n W[k][n] sum_b rows[n][b], no d_unit) riding
 * along as one extra workgroup of the same launch: the logged loss values cost no launch in the step's serial tail */
int mmvae_reduce_segments_lincomb(const mmvae_reduce_segments_t* table, const mmvae_rowptrs_t* rows,
                                  const float* W_host, float* out, int n_rows, int B, int n_out,
                                  mmvae_stream_t stream);
/* The fold and the optimiser step of a one-GPU training step as ONE launch: the gradient of element i is
 * g[i] + (sum of the registered partials that target it); every destination must lie inside [g, g + n), destination
 * ranges must not overlap (equal ranges are chained).  Same arithmetic, in the same order, as mmvae_reduce_segments
 * followed by mmvae_adam_amsgrad_flat(step = -1): bit-identical parameters and optimiser state.  step_dev as above
 * (the kernel advances it); rows == NULL: no ELBO assembly rider.  Replaces torch.optim.Adam.step()
 * (reference models/trainer.py:79-81) behind the backward pass's split weight gradients. */
int mmvae_adam_fold_flat(float* p, float* g, float* m, float* v, float* vmax, long n, float lr, float beta1,
                         float beta2, float eps, int* step_dev, float grad_scale, int zero_grad,
                         const mmvae_reduce_segments_t* table, const mmvae_rowptrs_t* rows, const float* W_host,
                         float* out, int n_rows, int B, int n_out, mmvae_stream_t stream);
/* One step's fold + update in SEVERAL launches: elements [lo, hi) of the flat buffers only (lo % 4 == 0), with those
 * segments of `table` whose destination lies inside the range (segments of another range of [0, n) are skipped; one that straddles lo
 * or hi, or whose destination is not wholly inside the flat buffer, is MMVAE_ERR_ARG; table may be NULL).  Every launch of a step reads the same step number from step_dev; exactly one --
 * the LAST in stream order -- passes advance_step = 1 and closes the step.  Per element bit-identical to
 * mmvae_adam_fold_flat over the whole buffer.  (The captured training step updates the decoders' + prior's range beside the
 * encoders' backward pass, so that only the encoders' parameters are left for the serial launch at the end of the step.)
 * Same reference interface as mmvae_adam_fold_flat: torch.optim.Adam.step(), models/trainer.py:79-81. */
int mmvae_adam_fold_range(float* p, float* g, float* m, float* v, float* vmax, long n, long lo, long hi,
                          int advance_step, float lr, float beta1, float beta2, float eps, int* step_dev,
                          float grad_scale, int zero_grad, const mmvae_reduce_segments_t* table,
                          const mmvae_rowptrs_t* rows, const float* W_host, float* out, int n_rows, int B, int n_out,
                          mmvae_stream_t stream);
/* partial layouts: rows x rowlen floats in ws; weight part at column 0, bias part at column bias_col */
int mmvae_conv_wgrad_layout(int B, int Csmall, int Clarge, int Hsmall, int* rows, int* rowlen, int* bias_col);
/* linear weight gradient: `splits` partial (N*K) slabs followed by `splits` partial (N) bias rows; splits == 1
 * means the kernel accumulated directly (nothing to reduce) */
int mmvae_linear_bwd_weight_splits(int M, int N, int K);
/* ... and by mmvae_linear_bwd (1 = written straight to dW/db: <= 256 rows with N % 4 == 0 take the register-operand
 * kernel, which needs dy 16-byte aligned) */
int mmvae_linear_bwd_splits(int M, int N, int K);
int mmvae_layernorm_bwd_rows(int rows, int d); /* partial rows of length 2*d: [dgamma | dbeta] */
int mmvae_embed_bwd_rows(int B, int T, int V);  /* partial rows of length 4 */

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_HIP_H */
