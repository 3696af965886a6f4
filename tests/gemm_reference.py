"""What tests/test_gemm_gpu.py measures the GEMM core (csrc/gemm.hip, gemm_b16.inc: mmvae_gemm_f32 and the nn.Linear
wrappers) against: a float64 restatement of the op written out from its definition, the case table with the kernel every
case is meant to reach, the deterministic inputs of every case, the per-element error bound and the part-by-part
comparison.  tests/test_gemm_reference_host.py pins the restatement to torch on the CPU, the case table and the split
mirrors to the library's own selector (mmvae_gemm_path / mmvae_linear_fwd_path / mmvae_linear_bwd_path, which launch
nothing) and shows that the checker catches seeded errors on exactly the part that carries them.

The op:  C[M,N] (+)= ep( bias[n] + sum_k act_a(A)[m,k] act_b(B)[k,n] ),  A(m,k) at A[m sam + k sak], B(k,n) at
B[k sbk + n sbn], C row-major with leading dimension ldc; rowsum[m] (+)= sum_k act_a(A)[m,k].  With nz > 1 reduction
splits of kper each and accumulate == ACC_DEFER the kernels leave raw partials in ws, [z][M][N] then [z][M], and C alone.

Conventions are the kernels' own: the ReLU mask is aux > 0 (so 0 and -0 mask), the clamp constants of EP_SIGMOID_CLAMP
are the float32 values of 1e-6 and 1 - 1e-6, gelu is the erf form, EP_GELU's aux RECEIVES bias + product."""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24                       # unit roundoff of float32
ACT_NONE, ACT_SILU, ACT_RELU, ACT_GELU = 0, 1, 2, 3
(EP_NONE, EP_RELU, EP_MUL_RELU_MASK, EP_MUL_SILU_GRAD, EP_GELU, EP_MUL_GELU_GRAD, EP_SIGMOID_CLAMP, EP_SIGMOID,
 EP_ADD_AUX) = range(9)
EP_READS_AUX = (EP_MUL_RELU_MASK, EP_MUL_SILU_GRAD, EP_MUL_GELU_GRAD, EP_ADD_AUX)
ACC_DEFER = 2
ERR_ARG, ERR_UNSUPPORTED = 1, 2
CLAMP_LO = float(torch.tensor(1e-6, dtype=torch.float32))
CLAMP_HI = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-6, dtype=torch.float32))


# kernel instantiations, by the names of include/mmvae_hip.h's enum without the MMVAE_GEMM_ prefix, in its order
_ORIENT = ("KK", "KN", "MK", "MN")      # A then B: K = reduction index contiguous, M / N = row / column index contiguous
_LOADS = ("VV", "VS", "SV", "SS")       # A then B: V = float4 along k, S = strided dwords
PATHS = (tuple(f"B16_{o}_{g}" for g in (1, 2) for o in _ORIENT) + tuple(f"BIG{bn}_{o}" for bn in (128, 64) for o in _ORIENT)
         + ("RSPLIT_16", "RSPLIT_64") + tuple(f"R{t}_{d}_{ld}" for t in (16, 32) for d in (16, 64) for ld in _LOADS)
         + tuple(f"STAGED{v}_{o}" for v in (1, 4, 8) for o in _ORIENT) + ("PROJ32", "LINBWD_B16_1", "LINBWD_B16_2")
         + ("LINBWD_R_16_T32", "LINBWD_R_16_T16", "LINBWD_R_64_T32", "LINBWD_R_64_T16", "LINBWD_STAGED", "LINBWD_TWO"))
PATH_VALUE = {name: 16 + i for i, name in enumerate(PATHS)}
PATH_NAME = {v: k for k, v in PATH_VALUE.items()}


# ---------------------------------------------------------------------------------------------
# the restatement (dtype of its inputs: float64 for the reference, float32 to measure e_fn)
# ---------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _cdf(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def silu(x):
    return x * _sigmoid(x)


def gelu(x):
    return x * _cdf(x)


def silu_grad(x):
    s = _sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


def gelu_grad(x):
    return _cdf(x) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def act(x, a):
    return {ACT_NONE: lambda t: t, ACT_SILU: silu, ACT_RELU: lambda t: t.clamp_min(0.0), ACT_GELU: gelu}[a](x)


def epilogue(v, aux, ep):
    """y = ep(v; aux)"""
    if ep == EP_NONE:
        return v
    if ep == EP_RELU:
        return v.clamp_min(0.0)
    if ep == EP_MUL_RELU_MASK:
        return torch.where(aux > 0, v, torch.zeros_like(v))
    if ep == EP_MUL_SILU_GRAD:
        return v * silu_grad(aux)
    if ep == EP_GELU:
        return gelu(v)
    if ep == EP_MUL_GELU_GRAD:
        return v * gelu_grad(aux)
    if ep == EP_SIGMOID_CLAMP:
        return _sigmoid(v).clamp(CLAMP_LO, CLAMP_HI)
    if ep == EP_SIGMOID:
        return _sigmoid(v)
    if ep == EP_ADD_AUX:
        return v + aux
    raise ValueError(ep)


def strided(flat, off, rows, cols, srow, scol):
    """the logical (rows, cols) operand of a flat buffer: element (r, c) at flat[off + r srow + c scol]"""
    return torch.as_strided(flat, (rows, cols), (srow, scol), off)


def split_ranges(K, nz, kper):
    return [(z * kper, min(K, (z + 1) * kper)) for z in range(nz)]


def gemm_reference(A, B, bias=None, aux=None, c_old=None, rs_old=None, a_act=ACT_NONE, b_act=ACT_NONE, ep=EP_NONE,
                   accumulate=0, rowsum=False, nz=1, kper=None):
    """A (M, K), B (K, N) logical operands -> dict of parts.  One split, or splits that the call itself reduces: "C", and
    "rowsum" / "aux" (EP_GELU with an aux buffer) where asked; accumulate adds the old contents.  Deferred splits
    (accumulate == ACC_DEFER, nz > 1): "partial" (nz, M, N) and "rs_partial" (nz, M), the sums over
    [z kper, min(K, (z + 1) kper)), and nothing else (C keeps its contents)."""
    a, b = act(A, a_act), act(B, b_act)
    K = A.shape[1]
    out = {}
    if nz > 1 and accumulate == ACC_DEFER:
        rng = split_ranges(K, nz, kper)
        out["partial"] = torch.stack([a[:, lo:hi] @ b[lo:hi] for lo, hi in rng])
        if rowsum:
            out["rs_partial"] = torch.stack([a[:, lo:hi].sum(1) for lo, hi in rng])
        return out
    v = a @ b
    if bias is not None:
        v = v + bias[None, :]
    if ep == EP_GELU and aux is not None:
        out["aux"] = v
    y = epilogue(v, aux, ep)
    out["C"] = y + c_old if accumulate else y
    if rowsum:
        rs = a.sum(1)
        out["rowsum"] = rs + rs_old if accumulate else rs
    return out


# The nn.Linear entry points, written out from that piece.  `_f` = gemm_reference (values) or gemm_bounds (their per-element
# bounds, with b16=...): one statement of each entry point serves both.
def _rename(r, names):
    return {names[k]: t for k, t in r.items()}


def linear_fwd_reference(x, w, b=None, aux=None, x_act=ACT_NONE, ep=EP_NONE, _f=None, **kw):
    """y = ep(act(x) W^T + b): x (M, K), w (N, K) -> "y" (and "aux" for EP_GELU with an aux buffer)"""
    return _rename((_f or gemm_reference)(x, w.t(), b, aux, a_act=x_act, ep=ep, **kw), {"C": "y", "aux": "aux"})


def linear_bwd_data_reference(dy, w, aux=None, dx_old=None, ep=EP_NONE, accumulate=0, _f=None, **kw):
    """dx (+)= ep(dy W; aux): dy (M, N), w (N, K)"""
    return _rename((_f or gemm_reference)(dy, w, None, aux, dx_old, ep=ep, accumulate=accumulate, **kw), {"C": "dx"})


def linear_bwd_weight_reference(dy, x, dw_old=None, db_old=None, x_act=ACT_NONE, accumulate=0, db=True, nz=1, kper=None,
                                _f=None, **kw):
    """dW (+)= dy^T act(x), db (+)= colsum(dy); deferred splits over the rows: "dw_partial" (nz, N, K), "db_partial" (nz, N)"""
    r = (_f or gemm_reference)(dy.t(), x, None, None, dw_old, db_old, b_act=x_act, accumulate=accumulate, rowsum=db, nz=nz,
                               kper=kper, **kw)
    return _rename(r, {"C": "dw", "rowsum": "db", "partial": "dw_partial", "rs_partial": "db_partial"})


def linear_bwd_reference(dy, x, w, aux=None, dw_old=None, db_old=None, x_act=ACT_NONE, ep=EP_NONE, accumulate=0, db=True,
                         nz=1, kper=None, _f=None, **kw):
    """the grouped backward: the data gradient (never accumulated) and the weight gradient of the same dy"""
    r = linear_bwd_data_reference(dy, w, aux, None, ep, 0, _f=_f, **kw)
    r.update(linear_bwd_weight_reference(dy, x, dw_old, db_old, x_act, accumulate, db, nz, kper, _f=_f, **kw))
    return r


# ---------------------------------------------------------------------------------------------
# error bounds, per element
# ---------------------------------------------------------------------------------------------
# of each part's own float64 maximum: what tests/test_hip_ops.py always asked of these kernels
CAP_FP32 = {"out": 2e-5, "grad": 5e-5, "db": 5e-5}
CAP_B16 = {"out": 3e-6, "grad": 3e-6, "db": 5e-6}
E_FN_MARGIN = 4.0
GELU_POLY_ERF_ERR = 1.5e-7      # csrc/gemm_b16.inc, gb_gelu: |erf error| of the Abramowitz-Stegun polynomial
LIPSCHITZ = {EP_NONE: 1.0, EP_RELU: 1.0, EP_GELU: 1.13, EP_SIGMOID: 0.25, EP_SIGMOID_CLAMP: 0.25, EP_ADD_AUX: 1.0}


def core_factor(k_red, b16):
    """the bound of a k_red-term dot product, in units of U sum_k |a_k| |b_k|.
    fp32 MFMA: any-order float32 accumulation of k_red rounded products is (k_red - 1 + 1) U to first order; + 2 for the
    bias and one more rounding; doubled because the MFMA's rounding inside its k pair is not documented as per-operation
    IEEE.
    split-bf16 (csrc/conv_gather_b16.inc): the three dropped terms are <= 3 U |a b|; the six kept bf16 x bf16 products
    are exact in float32 and accumulate in any order: 6 k_red terms whose magnitudes sum to <= (1 + 2^-7)^2 |a| |b|
    (|x0| + |x1| + |x2| <= (1 + 2^-7) |x| for truncated 8-bit terms), with the same + 2 and the same doubling."""
    if b16:
        return 3.0 + 2.0 * (6 * k_red + 2) * (1.0 + 2.0 ** -7) ** 2
    return 2.0 * (k_red + 2)


def _fn_err(fn, x, floor):
    """E_FN_MARGIN x the error of the float32 torch-CPU evaluation of fn against its float64 evaluation on these very
    inputs, element by element, never below `floor`: the error that the function's last float32 operation has by the
    number format alone (an element where the float32 evaluation happens to round to the float64 value would otherwise
    allow the hardware's exp / rcp nothing).  Never calibrated from a kernel's output."""
    x = x.to(F64)
    measured = (fn(x.float()).to(F64) - fn(x)).abs()
    return E_FN_MARGIN * torch.maximum(measured, floor)


def act_err(x, a, b16=False):
    """error allowed on act(x), elementwise.  silu = x sigmoid(x) and gelu = x Phi(x): the factor in (0, 1) is good to U
    absolutely in float32, hence the floor U |x|.  The polynomial GELU of the split-bf16 kernel adds its stated erf error."""
    x = x.to(F64)
    if a in (ACT_NONE, ACT_RELU):
        return torch.zeros_like(x)
    e = _fn_err(silu if a == ACT_SILU else gelu, x, U * x.abs())
    if a == ACT_GELU and b16:
        e = e + 0.5 * x.abs() * GELU_POLY_ERF_ERR
    return e


def ep_fn_err(v, aux, ep):
    """error allowed on the epilogue's own function at exact arguments (v: float64 pre-activation)"""
    v = v.to(F64)
    if ep == EP_GELU:
        return _fn_err(gelu, v.float(), U * v.abs())
    if ep in (EP_SIGMOID, EP_SIGMOID_CLAMP):
        return _fn_err(_sigmoid, v.float(), torch.full_like(v, U))
    if ep in (EP_MUL_SILU_GRAD, EP_MUL_GELU_GRAD):      # derivative = factor in (0, 1) + x times one: U (1 + |x|)
        f = silu_grad if ep == EP_MUL_SILU_GRAD else gelu_grad
        return v.abs() * _fn_err(f, aux, U * (1.0 + aux.to(F64).abs()))
    return torch.zeros_like(v)


def gemm_bounds(A, B, bias=None, aux=None, c_old=None, rs_old=None, a_act=ACT_NONE, b_act=ACT_NONE, ep=EP_NONE,
                accumulate=0, rowsum=False, nz=1, kper=None, b16=False):
    """per-element bound of every part gemm_reference returns for the same arguments:
         |got - ref| <= core_factor(K_red) U (|act(A)| |act(B)| + |bias|)[m,n] + e_fn
    carried through the epilogue by its Lipschitz constant (or |f'(aux)| for the MUL_* forms), plus two roundings of the
    stored value and, when accumulating, one of old + new.  e_fn: the operand activations' error carried through the
    product, and the epilogue function's own."""
    A, B = A.to(F64), B.to(F64)
    a, b = act(A, a_act), act(B, b_act)
    ea, eb = act_err(A, a_act, b16), act_err(B, b_act, b16)
    K = A.shape[1]
    out = {}

    def dot_bound(lo, hi):
        mag = a[:, lo:hi].abs() @ b[lo:hi].abs()
        e_in = torch.zeros_like(mag)
        if a_act in (ACT_SILU, ACT_GELU):
            e_in = e_in + ea[:, lo:hi] @ b[lo:hi].abs()
        if b_act in (ACT_SILU, ACT_GELU):
            e_in = e_in + (a[:, lo:hi].abs() + ea[:, lo:hi]) @ eb[lo:hi]
        return mag, e_in

    def rs_bound(lo, hi):
        return 2.0 * (hi - lo + 2) * U * a[:, lo:hi].abs().sum(1) + ea[:, lo:hi].sum(1)

    if nz > 1 and accumulate == ACC_DEFER:
        rng = split_ranges(K, nz, kper)
        parts = []
        for lo, hi in rng:
            mag, e_in = dot_bound(lo, hi)
            parts.append(core_factor(hi - lo, b16) * U * mag + e_in)
        out["partial"] = torch.stack(parts)
        if rowsum:
            out["rs_partial"] = torch.stack([rs_bound(lo, hi) for lo, hi in rng])
        return out
    mag, e_in = dot_bound(0, K)
    v = a @ b
    if bias is not None:
        v = v + bias.to(F64)[None, :]
        mag = mag + bias.to(F64).abs()[None, :]
    bv = core_factor(K, b16) * U * mag + e_in
    if ep == EP_GELU and aux is not None:
        out["aux"] = bv
    y = epilogue(v, None if aux is None else aux.to(F64), ep)
    if ep == EP_MUL_RELU_MASK:
        by = torch.where(aux > 0, bv, torch.zeros_like(bv))
    elif ep == EP_MUL_SILU_GRAD:
        by = silu_grad(aux.to(F64)).abs() * bv
    elif ep == EP_MUL_GELU_GRAD:
        by = gelu_grad(aux.to(F64)).abs() * bv
    else:
        by = LIPSCHITZ[ep] * bv
    by = by + ep_fn_err(v, aux, ep) + 2.0 * U * y.abs()
    if accumulate:
        by = by + U * (c_old.to(F64).abs() + y.abs())
    out["C"] = by
    if rowsum:
        rb = rs_bound(0, K)
        if accumulate:
            rb = rb + U * (rs_old.to(F64).abs() + a.sum(1).abs())
        out["rowsum"] = rb
    return out


def part_kind(part):
    return "db" if part in ("db", "rowsum", "db_partial", "rs_partial") else "out" if part in ("C", "y", "aux") else "grad"


def gemm_part_kind(case, part):
    """which of the suite's max-norm tolerances a part of a case falls under: outputs 2e-5, gradients 5e-5 (split-bf16:
    3e-6, bias gradient 5e-6)"""
    if part in ("db", "rowsum", "db_partial", "rs_partial"):
        return "db"
    if case.entry in ("gemm", "linear_fwd"):
        return "out"
    return "grad"


def check_part(name, got, ref, bound, cap):
    """both checks of one part; got float32 (or float64 holding float32 values), ref / bound float64.
    -> (ok, ratio of the worst error to the max-norm tolerance, worst ratio of an element's error to its bound, message)"""
    got, ref, bound = got.to(F64), ref.to(F64), bound.to(F64)
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    if not bool(torch.isfinite(got).all()):
        return False, math.inf, math.inf, f"{name}: non-finite values"
    err = (got - ref).abs()
    scale = max(float(ref.abs().max()), 1e-30)
    r_max = float(err.max()) / (cap * scale)
    # an element whose bound is 0 (a masked one) must be exact
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                                 torch.zeros_like(err)))
    r_el = float(ratio.max())
    msg = ""
    if r_max > 1.0:
        msg = f"{name}: max error {float(err.max()):.3e} is {r_max:.2f} x the max-norm tolerance {cap:g} of {scale:.3e}"
    elif r_el > 1.0:
        i = int(ratio.argmax())
        msg = (f"{name}: element {i} is off by {float(err.flatten()[i]):.3e}, {r_el:.2f} x its bound "
               f"{float(bound.flatten()[i]):.3e} (value {float(ref.flatten()[i]):.6e})")
    return r_max <= 1.0 and r_el <= 1.0, r_max, r_el, msg


def check_parts(case, got, ref, bounds, b16=False):
    """-> {part: (ok, r_max, r_el, message)} over every part of ref (got must hold them all)"""
    cap = CAP_B16 if b16 else CAP_FP32
    assert set(got) == set(ref) == set(bounds), (sorted(got), sorted(ref), sorted(bounds))
    return {p: check_part(p, got[p], ref[p], bounds[p], cap[gemm_part_kind(case, p)]) for p in ref}


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
ENTRIES = ("gemm", "linear_fwd", "bwd_data", "bwd_weight", "linear_bwd")
GUARD = 64          # floats of guard band on either side of every device buffer (a multiple of 4: keeps 16-byte alignment)


class Case:
    """one call recipe and the kernel it is meant to reach: `path` with the split-bf16 core on, `path0` with it off.

    entry "gemm": mmvae_gemm_f32 of C (M, N) = A (M, K) B (K, N); orient gives the contiguous index of A then B; pad_a /
      pad_b widen the operands' leading dimensions, off_a / off_b shift their base by that many floats (1 = 4-byte but
      not 16-byte aligned), ldc = N + ldc_pad.
    entry "linear_fwd" / "bwd_data" / "bwd_weight" / "linear_bwd": nn.Linear with M rows, K inputs, N outputs.  pad_a is
      the padding of ldx, a_act the activation on x, off_a the offset of the FIRST operand of the call (x / dy / dy / dy),
      off_b of its second (w / w / x / x); rowsum = "with db"; acc the accumulate argument."""

    def __init__(self, entry, M, N, K, path, path0=None, orient="KK", pad_a=0, pad_b=0, off_a=0, off_b=0, ldc_pad=0,
                 a_act=ACT_NONE, b_act=ACT_NONE, ep=EP_NONE, bias=False, rowsum=False, acc=0, splitk=1, aux_write=True):
        assert entry in ENTRIES and orient in _ORIENT and path in PATHS and (path0 is None or path0 in PATHS)
        assert not (splitk > 1 and (bias or ep != EP_NONE)), "the call refuses a split with a bias or an epilogue"
        assert entry == "gemm" or (orient == "KK" and pad_b == 0 and ldc_pad == 0 and b_act == ACT_NONE and splitk == 1)
        self.entry, self.M, self.N, self.K, self.path, self.path0 = entry, M, N, K, path, path0 or path
        self.orient, self.pad_a, self.pad_b, self.off_a, self.off_b, self.ldc_pad = orient, pad_a, pad_b, off_a, off_b, ldc_pad
        self.a_act, self.b_act, self.ep, self.bias, self.rowsum, self.acc, self.splitk = a_act, b_act, ep, bias, rowsum, acc, splitk
        self.aux_write = aux_write and ep == EP_GELU
        self.name = (f"{entry}-{M}x{N}x{K}-{orient}-p{pad_a}.{pad_b}-o{off_a}.{off_b}-c{ldc_pad}-a{a_act}.{b_act}-e{ep}"
                     f"{'-bias' if bias else ''}{'-rs' if rowsum else ''}-acc{acc}-s{splitk}{'' if aux_write else '-noaux'}")

    def __repr__(self):
        return self.name

    def strides(self):
        """entry "gemm": sam, sak, sbk, sbn, ldc"""
        sam, sak = (self.K + self.pad_a, 1) if self.orient[0] == "K" else (1, self.M + self.pad_a)
        sbk, sbn = (1, self.K + self.pad_b) if self.orient[1] == "K" else (self.N + self.pad_b, 1)
        return sam, sak, sbk, sbn, self.N + self.ldc_pad

    @property
    def ldx(self):
        return self.K + self.pad_a

    def query(self, lib, al_a=None, al_b=None, al_c=True):
        """the library's own selector for this call -> (path value or negated error, nz, kper).  al_*: is the pointer
        16-byte aligned (default: what the offsets give inside a 16-byte aligned buffer)"""
        import ctypes
        al_a = self.off_a == 0 if al_a is None else al_a
        al_b = self.off_b == 0 if al_b is None else al_b
        nz, kper = ctypes.c_int(1), ctypes.c_int(0)
        out = (ctypes.byref(nz), ctypes.byref(kper))
        M, N, K = self.M, self.N, self.K
        if self.entry == "gemm":
            p = lib.mmvae_gemm_path(M, N, K, *self.strides(), self.a_act, self.b_act, self.ep, self.acc, self.splitk,
                                    int(self.rowsum), int(al_a), int(al_b), *out)
        elif self.entry == "linear_fwd":
            p = lib.mmvae_linear_fwd_path(M, N, K, self.ldx, self.a_act, self.ep, int(al_a), int(al_b), int(al_c))
            kper.value = K
        elif self.entry == "bwd_data":       # dx (M, K) = dy (M, N) W (N, K)
            p = lib.mmvae_gemm_path(M, K, N, N, 1, K, 1, K, ACT_NONE, ACT_NONE, self.ep, self.acc, 1, 0, int(al_a), int(al_b), *out)
        elif self.entry == "bwd_weight":
            p = lib.mmvae_linear_bwd_weight_path(M, N, K, self.ldx, self.a_act, self.acc, int(self.rowsum), int(al_a), int(al_b), *out)
        else:
            p = lib.mmvae_linear_bwd_path(M, N, K, self.ldx, self.a_act, self.ep, self.acc, int(self.rowsum), int(al_a),
                                          int(al_b), int(al_c), *out)
        return p, nz.value, kper.value

    # the reduction length and the ragged dimensions, for the coverage assertions of the host test
    def reductions(self):
        return {"gemm": (self.K,), "linear_fwd": (self.K,), "bwd_data": (self.N,), "bwd_weight": (self.M,),
                "linear_bwd": (self.N, self.M)}[self.entry]


_SPECIAL = (0.0, 6.0, -6.0, 0.0, 20.0, -20.0, 0.0)      # exact zeros and tails of SiLU / GELU / sigmoid
_SPECIAL_AUX = (0.0, -0.0, 10.0, -10.0, 0.0, -0.0, 4.0, -4.0)


def _poke(t, values):
    """scatter `values` over t at fixed, spread positions (fewer of them into a tensor too small to stay random)"""
    flat = t.view(-1)
    n = flat.numel()
    for i, v in enumerate(values[: max(1, min(len(values), n // 3))]):
        flat[(i * 7919 + n // 2) % n] = v
    return t


def make_inputs(case):
    """-> dict of contiguous float32 CPU tensors, the logical operands of the call (the layout is the test's business).
    Seeded normal values; exact zeros and +-6, +-20 in the operands; aux holds 0 and -0 (the ReLU mask's edge) and +-10"""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    M, N, K, e = case.M, case.N, case.K, case.entry

    def rnd(*shape, scale=1.0, special=_SPECIAL):
        return _poke(torch.randn(*shape, generator=g) * scale, special)

    d = {}
    if e == "gemm":
        d["A"], d["B"] = rnd(M, K), rnd(K, N, scale=1.0 / math.sqrt(K))
        out_shape, red = (M, N), None
        if case.rowsum and case.acc:
            d["rs_old"] = rnd(M, special=())
    elif e == "linear_fwd":
        d["x"], d["w"] = rnd(M, K), rnd(N, K, scale=1.0 / math.sqrt(K))
        out_shape = (M, N)
    else:
        d["dy"] = rnd(M, N)
        if e != "bwd_weight":
            d["w"] = rnd(N, K, scale=1.0 / math.sqrt(N))
        if e != "bwd_data":
            d["x"] = rnd(M, K)
            if case.acc:
                d["dw_old"] = rnd(N, K, special=())
                if case.rowsum:
                    d["db_old"] = rnd(N, special=())
        out_shape = (M, K)
    if case.bias:
        d["bias"] = rnd(N, scale=0.5, special=(0.0,))
    if case.ep in EP_READS_AUX:
        d["aux"] = rnd(*out_shape, special=_SPECIAL_AUX)
    if case.acc and e in ("gemm", "bwd_data"):
        d["c_old" if e == "gemm" else "dx_old"] = rnd(*out_shape, special=())
    return d


def expected(case, inp, nz=1, kper=None, b16=False):
    """-> (ref, bounds): the float64 parts of the call on these inputs and their per-element bounds"""
    d = {k: v.to(F64) for k, v in inp.items()}
    c, e = case, case.entry
    aux = d.get("aux")
    res = []
    for f, extra in ((gemm_reference, {}), (gemm_bounds, {"b16": b16})):
        if e == "gemm":
            # EP_GELU writes aux only when given a buffer: the reference then takes a placeholder
            a_ = aux if c.ep in EP_READS_AUX else (d["A"][:0] if c.aux_write else None)
            r = f(d["A"], d["B"], d.get("bias"), a_, d.get("c_old"), d.get("rs_old"), c.a_act, c.b_act, c.ep, c.acc, c.rowsum,
                  nz, kper, **extra)
        elif e == "linear_fwd":
            a_ = d["x"][:0] if c.aux_write else None
            r = linear_fwd_reference(d["x"], d["w"], d.get("bias"), a_, c.a_act, c.ep, _f=f, **extra)
        elif e == "bwd_data":
            r = linear_bwd_data_reference(d["dy"], d["w"], aux, d.get("dx_old"), c.ep, c.acc, _f=f, **extra)
        elif e == "bwd_weight":
            r = linear_bwd_weight_reference(d["dy"], d["x"], d.get("dw_old"), d.get("db_old"), c.a_act, c.acc, c.rowsum, nz,
                                            kper, _f=f, **extra)
        else:
            r = linear_bwd_reference(d["dy"], d["x"], d["w"], aux, d.get("dw_old"), d.get("db_old"), c.a_act, c.ep, c.acc,
                                     c.rowsum, nz, kper, _f=f, **extra)
        res.append(r)
    return res[0], res[1]


def _g(*a, **k):
    return Case("gemm", *a, **k)


DEFER = ACC_DEFER
# The smallest shapes that reach each instantiation, ragged in every dimension the path allows: a last tile of one row /
# column (or of four, where the float4 staging of a row-contiguous operand needs the dimension % 4 == 0), a reduction
# that is no multiple of the stage depth, a last split shorter than kper.  tests/test_gemm_reference_host.py asks the
# library's selector for every one of them.
CASES = (
    # ---- staged kernel, 128 x 32 tiles: >= 256 of them, and (one split) > 1024 32 x 32 tiles or the register kernel runs
    _g(1025, 993, 6, "STAGED1_KK", ep=EP_RELU, bias=True, ldc_pad=3),
    _g(1025, 993, 6, "STAGED1_KN", orient="KN", ep=EP_SIGMOID, bias=True, pad_b=1),
    _g(1025, 993, 6, "STAGED1_MK", orient="MK", ep=EP_ADD_AUX, acc=1, pad_a=2),
    _g(1025, 993, 6, "STAGED1_MN", orient="MN", rowsum=True, a_act=ACT_SILU, ldc_pad=3),
    _g(1025, 993, 130, "STAGED1_KK", splitk=3, rowsum=True, acc=DEFER),                       # splits of 64, 64, 2
    # ---- staged kernel, 32 x 32 tiles over 8 waves: one split, K > 1024, few tiles
    _g(33, 33, 1029, "STAGED8_KK", ep=EP_GELU, bias=True),
    _g(40, 33, 1028, "STAGED8_KN", orient="KN", ep=EP_MUL_RELU_MASK, ldc_pad=3),
    _g(33, 40, 1030, "STAGED8_MK", orient="MK", ep=EP_SIGMOID_CLAMP, bias=True),
    _g(33, 33, 1029, "STAGED8_MN", orient="MN", rowsum=True, acc=1, b_act=ACT_RELU),
    _g(1, 1, 1030, "STAGED8_KK"),
    # ---- staged kernel, 32 x 32 tiles over 4 waves: any split request on a k-major operand, or splits longer than 1024
    _g(33, 33, 300, "STAGED4_KK", splitk=3, acc=DEFER, ldc_pad=3),                              # 128, 128, 44; C untouched
    _g(33, 17, 300, "STAGED4_KN", orient="KN", splitk=3),
    _g(17, 33, 300, "STAGED4_MK", orient="MK", splitk=3, rowsum=True, acc=1, a_act=ACT_GELU),
    _g(33, 33, 2500, "STAGED4_MN", orient="MN", splitk=2, rowsum=True, acc=DEFER),              # 1280, 1220
    _g(65, 5441, 1028, "STAGED4_KK", ep=EP_RELU, bias=True),                                     # one split: > 512 tiles, K > 1024
    # ---- register-operand kernel with a split reduction (weight gradients with few tiles): m-major A, n-major B only
    _g(33, 17, 300, "RSPLIT_16", orient="MN", splitk=3, rowsum=True, acc=DEFER, b_act=ACT_SILU),
    _g(17, 33, 300, "RSPLIT_16", orient="MN", splitk=3, rowsum=True),
    _g(33, 17, 1000, "RSPLIT_64", orient="MN", splitk=2, rowsum=True, acc=1),                    # 512, 488
    _g(2, 1, 1000, "RSPLIT_64", orient="MN", splitk=2, acc=DEFER),
    # ---- register-operand kernel, 16 x 16 tiles: <= 128 32 x 32 tiles, no row sum, K <= 1024; 16 deep below K = 384
    _g(17, 33, 20, "R16_16_VV", ep=EP_RELU, bias=True, ldc_pad=3),
    _g(17, 33, 20, "R16_16_VS", orient="KN", ep=EP_GELU, bias=True),
    _g(17, 33, 20, "R16_16_VS", off_b=1, ep=EP_GELU, aux_write=False),                          # k-major B off 16 bytes
    _g(17, 33, 20, "R16_16_SV", orient="MK", ep=EP_SIGMOID, bias=True),
    _g(17, 33, 20, "R16_16_SV", off_a=1, ep=EP_MUL_GELU_GRAD),
    _g(17, 33, 21, "R16_16_SS", ep=EP_MUL_SILU_GRAD, a_act=ACT_SILU),                            # K % 4 != 0
    _g(17, 33, 20, "R16_16_SS", pad_a=1, pad_b=2, acc=1),                                        # row strides % 4 != 0
    _g(33, 17, 20, "R16_16_SS", orient="MN", ep=EP_MUL_RELU_MASK, ldc_pad=3),
    _g(5, 7, 1, "R16_16_SS"),                                                                   # K = 1: sbn == 1 reads as n-major
    _g(1, 1, 1, "R16_16_SS", bias=True),
    _g(17, 33, 388, "R16_64_VV", ep=EP_SIGMOID_CLAMP, bias=True),
    _g(33, 17, 388, "R16_64_VS", orient="KN", ep=EP_ADD_AUX, ldc_pad=3),
    _g(17, 33, 388, "R16_64_SV", orient="MK", ep=EP_RELU, a_act=ACT_RELU),
    _g(17, 33, 385, "R16_64_SS", acc=1, ep=EP_GELU, bias=True),
    _g(33, 17, 1021, "R16_64_SS", orient="MN", b_act=ACT_GELU),
    # ---- register-operand kernel, 32 x 32 tiles: a row sum, or 129 .. 1024 tiles
    _g(33, 17, 20, "R32_16_VV", rowsum=True, a_act=ACT_GELU, ep=EP_RELU, bias=True),
    _g(17, 33, 20, "R32_16_VS", orient="KN", rowsum=True, acc=1, ldc_pad=3),
    _g(33, 17, 20, "R32_16_SV", orient="MK", rowsum=True, a_act=ACT_SILU, ep=EP_SIGMOID),
    _g(33, 17, 21, "R32_16_SS", rowsum=True, ep=EP_MUL_RELU_MASK),
    _g(353, 353, 20, "R32_16_VV", ep=EP_GELU, bias=True),                                        # 144 tiles, no row sum
    _g(1, 1, 5, "R32_16_SS", rowsum=True),
    _g(33, 17, 388, "R32_64_VV", rowsum=True, ep=EP_MUL_SILU_GRAD),
    _g(17, 33, 388, "R32_64_VS", orient="KN", rowsum=True, a_act=ACT_RELU, ldc_pad=3),
    _g(33, 17, 388, "R32_64_SV", orient="MK", rowsum=True, acc=1),
    _g(17, 33, 1021, "R32_64_SS", orient="MN", rowsum=True, b_act=ACT_SILU, acc=DEFER),          # DEFER, one split: accumulates
    # ---- large-tile kernel, 128 x 64: >= 384 tiles x splits, float4-loadable operands, outside the split-bf16 window
    _g(1921, 1473, 20, "BIG64_KK", ep=EP_RELU, bias=True, ldc_pad=3),
    _g(1921, 1476, 20, "BIG64_KN", orient="KN", ep=EP_SIGMOID_CLAMP, bias=True, pad_b=4),
    _g(1924, 1473, 20, "BIG64_MK", orient="MK", ep=EP_MUL_GELU_GRAD, pad_a=4),
    _g(1924, 1476, 21, "BIG64_MN", orient="MN", rowsum=True, acc=1, a_act=ACT_SILU),
    _g(1924, 1476, 68, "BIG64_MN", orient="MN", splitk=2, rowsum=True, acc=DEFER),              # 64, 4
    # ---- large-tile kernel, 128 x 128: >= 512 tiles x splits
    _g(3969, 1921, 16, "BIG128_KK", ep=EP_RELU, bias=True),
    _g(1921, 1924, 68, "BIG128_KN", orient="KN", splitk=2),
    _g(1924, 1921, 68, "BIG128_MK", orient="MK", splitk=2, rowsum=True, acc=1),
    _g(1924, 1924, 68, "BIG128_MN", orient="MN", splitk=2, rowsum=True, acc=DEFER, b_act=ACT_RELU),
    # ---- LDS-tiled split-bf16 kernel: 2048 .. 4096 rows, N, K >= 128 and % 4 == 0, one split, no row sum, not EP_GELU;
    #      two k-groups below 256 tiles when K >= 256
    _g(2048, 128, 128, "B16_KK_1", "R32_16_VV"),
    _g(2049, 132, 132, "B16_KK_1", "R32_16_VV", ep=EP_RELU, bias=True, ldc_pad=3),
    _g(2049, 132, 132, "B16_KN_1", "R32_16_VS", orient="KN", ep=EP_MUL_SILU_GRAD, pad_a=4),
    _g(2052, 132, 132, "B16_MK_1", "R32_16_SV", orient="MK", a_act=ACT_SILU, ep=EP_SIGMOID, bias=True),
    _g(2052, 132, 132, "B16_MN_1", "R32_16_SS", orient="MN", b_act=ACT_GELU, acc=1, pad_b=4),
    _g(2049, 132, 260, "B16_KK_2", "R32_16_VV", ep=EP_SIGMOID_CLAMP, bias=True),
    _g(2049, 132, 260, "B16_KN_2", "R32_16_VS", orient="KN", ep=EP_ADD_AUX, a_act=ACT_GELU),
    _g(2052, 132, 260, "B16_MK_2", "R32_16_SV", orient="MK", ep=EP_MUL_RELU_MASK, ldc_pad=3),
    _g(2052, 132, 260, "B16_MN_2", "R32_16_SS", orient="MN", a_act=ACT_RELU, ep=EP_MUL_GELU_GRAD, acc=DEFER),
    # ---- nn.Linear forward
    Case("linear_fwd", 1025, 96, 32, "PROJ32", bias=True),
    Case("linear_fwd", 1025, 32, 32, "PROJ32"),
    Case("linear_fwd", 17, 33, 20, "R16_16_VV", pad_a=4, a_act=ACT_SILU, ep=EP_GELU, bias=True),       # ldx != K
    Case("linear_fwd", 17, 33, 20, "R16_16_SV", pad_a=1, ep=EP_GELU, bias=True, aux_write=False),
    Case("linear_fwd", 2049, 132, 132, "B16_KK_1", "R32_16_VV", a_act=ACT_RELU, ep=EP_SIGMOID, bias=True),
    # ---- data gradient (A = dy k-major, B = W n-major); accumulate = 1 is the recurrent layer's use
    Case("bwd_data", 17, 20, 33, "R16_16_VS", ep=EP_MUL_RELU_MASK, acc=1),
    Case("bwd_data", 17, 21, 33, "R16_16_SS", acc=1),
    Case("bwd_data", 2049, 132, 132, "B16_KN_1", "R32_16_VS", acc=1, ep=EP_MUL_SILU_GRAD),
    # ---- weight gradient alone (A = dy m-major, B = x n-major): without db and one split it moves to 16 x 16 tiles
    Case("bwd_weight", 100, 17, 33, "R16_16_SS", a_act=ACT_SILU),
    Case("bwd_weight", 100, 17, 33, "R32_16_SS", rowsum=True, acc=1, pad_a=3),
    Case("bwd_weight", 300, 17, 33, "RSPLIT_16", rowsum=True, a_act=ACT_RELU),
    Case("bwd_weight", 300, 17, 33, "RSPLIT_16", rowsum=True, acc=DEFER),
    # ---- grouped backward
    Case("linear_bwd", 17, 20, 33, "LINBWD_R_16_T16", rowsum=True, ep=EP_MUL_SILU_GRAD, a_act=ACT_SILU, acc=1, pad_a=3),
    Case("linear_bwd", 353, 20, 353, "LINBWD_R_16_T32", rowsum=True),
    Case("linear_bwd", 17, 388, 33, "LINBWD_R_64_T16", ep=EP_ADD_AUX),
    Case("linear_bwd", 353, 388, 353, "LINBWD_R_64_T32", rowsum=True, ep=EP_MUL_RELU_MASK, a_act=ACT_RELU),
    Case("linear_bwd", 300, 5, 17, "LINBWD_STAGED", rowsum=True, acc=DEFER),                          # 128, 128, 44 rows
    Case("linear_bwd", 33, 5, 17, "LINBWD_STAGED", rowsum=True, acc=1, ep=EP_MUL_GELU_GRAD, a_act=ACT_GELU),
    Case("linear_bwd", 2049, 5, 481, "LINBWD_TWO", rowsum=True),
    Case("linear_bwd", 2049, 132, 132, "LINBWD_B16_1", "LINBWD_STAGED", rowsum=True, acc=DEFER),
    Case("linear_bwd", 2049, 256, 132, "LINBWD_B16_2", "LINBWD_STAGED", rowsum=True, acc=1, ep=EP_MUL_RELU_MASK, a_act=ACT_RELU),
)
# Instantiations no supported call reaches.  None today: every family takes all four operand forms through
# mmvae_gemm_f32 (the A-m-major / B-k-major one through the C ABI only), so an entry here needs its reason beside it.
UNREACHABLE = ()


# ---------------------------------------------------------------------------------------------
# memory layout of a call: every buffer sits inside a larger one filled with a sentinel
# ---------------------------------------------------------------------------------------------
SENTINEL = 0x7FA5A5A5       # a quiet NaN: a padding element that leaks into a sum, or an element left unwritten, shows
PAST_ROWS = 2               # rows past the matrix, inside the buffer


class Buf:
    """a row-major (rows, cols) matrix with leading dimension ld, `off` floats past a 16-byte aligned address, inside a
    flat buffer of sentinels: [GUARD | off | rows + PAST_ROWS rows of ld | GUARD].  data: the logical contents (None: the
    matrix itself starts as sentinels, as an output that the call must overwrite entirely)"""

    def __init__(self, rows, cols, ld=None, off=0, data=None, device="cpu"):
        self.rows, self.cols, self.ld, self.off = rows, cols, ld or cols, off
        assert self.ld >= cols
        n = 2 * GUARD + off + (rows + PAST_ROWS) * self.ld
        flat = torch.full((n,), SENTINEL, dtype=torch.int32).view(torch.float32)
        if data is not None:
            assert tuple(data.shape) == (rows, cols), (data.shape, rows, cols)
            torch.as_strided(flat, (rows, cols), (self.ld, 1), GUARD + off).copy_(data)
        self.flat = flat.to(device)
        self.before = self.flat.clone()

    @property
    def ptr(self):
        return self.flat.data_ptr() + 4 * (GUARD + self.off)

    @property
    def aligned16(self):
        return self.ptr % 16 == 0

    def view(self, flat=None):
        return torch.as_strided(self.flat if flat is None else flat, (self.rows, self.cols), (self.ld, 1), GUARD + self.off)

    def outside_intact(self):
        """everything but the matrix itself (guard bands, padding columns, rows past the end) is bit-identical"""
        now, was = self.flat.clone().view(torch.int32), self.before.clone().view(torch.int32)
        self.view(now).zero_()
        self.view(was).zero_()
        return bool(torch.equal(now, was))

    def intact(self, first=0):
        """bit-identical from flat element `first` of the matrix region on (0: the whole buffer)"""
        a, b = self.flat.view(torch.int32), self.before.view(torch.int32)
        return bool(torch.equal(a[GUARD + self.off + first:], b[GUARD + self.off + first:])) and \
            bool(torch.equal(a[:GUARD + self.off], b[:GUARD + self.off]))


def out_dims(case):
    """(rows, cols, ld) of the call's main output and of its weight-gradient output (or None)"""
    M, N, K = case.M, case.N, case.K
    if case.entry == "gemm":
        return (M, N, N + case.ldc_pad), None
    if case.entry == "linear_fwd":
        return (M, N, N), None
    if case.entry == "bwd_data":
        return (M, K, K), None
    if case.entry == "bwd_weight":
        return None, (N, K, K)
    return (M, K, K), (N, K, K)


def split_dims(case):
    """(rows, cols) of the problem whose reduction the call splits: partials are nz x (rows cols [+ rows]) floats of ws"""
    return (case.M, case.N) if case.entry == "gemm" else (case.N, case.K)


def build_buffers(case, inp, ws_floats, device="cpu"):
    """-> {name: Buf} of every pointer the call takes.  Outputs that the call must overwrite start as sentinels; those it
    accumulates into start from the non-constant old contents."""
    M, N, K, e = case.M, case.N, case.K, case.entry
    b = {}
    mk = lambda rows, cols, ld=None, off=0, data=None: Buf(rows, cols, ld, off, data, device)
    main, wg = out_dims(case)
    if e == "gemm":
        A, B = inp["A"], inp["B"]
        b["A"] = mk(M, K, K + case.pad_a, case.off_a, A) if case.orient[0] == "K" else mk(K, M, M + case.pad_a, case.off_a, A.t())
        b["B"] = mk(N, K, K + case.pad_b, case.off_b, B.t()) if case.orient[1] == "K" else mk(K, N, N + case.pad_b, case.off_b, B)
        b["C"] = mk(*main, data=inp.get("c_old"))
        if case.rowsum:
            b["rowsum"] = mk(1, M, data=inp["rs_old"][None] if "rs_old" in inp else None)
    elif e == "linear_fwd":
        b["x"], b["w"] = mk(M, K, case.ldx, case.off_a, inp["x"]), mk(N, K, K, case.off_b, inp["w"])
        b["y"] = mk(*main)
    else:
        b["dy"] = mk(M, N, N, case.off_a, inp["dy"])
        if e != "bwd_weight":
            b["w"] = mk(N, K, K, case.off_b if e == "bwd_data" else 0, inp["w"])
            b["dx"] = mk(*main, data=inp.get("dx_old"))
        if e != "bwd_data":
            b["x"] = mk(M, K, case.ldx, case.off_b, inp["x"])
            b["dw"] = mk(*wg, data=inp.get("dw_old"))
            if case.rowsum:
                b["db"] = mk(1, N, data=inp["db_old"][None] if "db_old" in inp else None)
    if case.bias:
        b["bias"] = mk(1, N, data=inp["bias"][None])
    if case.ep in EP_READS_AUX or case.aux_write:
        b["aux"] = mk(main[0], main[1], main[2], data=inp.get("aux"))
    if e in ("gemm", "bwd_weight", "linear_bwd"):
        b["ws"] = mk(1, max(int(ws_floats), 4))
    return b


OUTPUTS = {"gemm": {"C": "C", "rowsum": "rowsum"}, "linear_fwd": {"y": "y"}, "bwd_data": {"dx": "dx"},
           "bwd_weight": {"dw": "dw", "db": "db"}, "linear_bwd": {"dx": "dx", "dw": "dw", "db": "db"}}
_PARTIALS = {"gemm": ("partial", "rs_partial", "C", "rowsum"), "bwd_weight": ("dw_partial", "db_partial", "dw", "db"),
             "linear_bwd": ("dw_partial", "db_partial", "dw", "db")}


def deferred(case, nz):
    return nz > 1 and case.acc == ACC_DEFER


def collect(case, bufs, nz):
    """-> the parts the call produced, as float32 CPU tensors shaped like the reference's"""
    got = {}
    if deferred(case, nz):
        pw, pr, cw, cr = _PARTIALS[case.entry]
        rows, cols = split_dims(case)
        ws = bufs["ws"].view().cpu().reshape(-1)
        got[pw] = ws[: nz * rows * cols].reshape(nz, rows, cols).clone()
        if case.rowsum:
            got[pr] = ws[nz * rows * cols: nz * (rows * cols + rows)].reshape(nz, rows).clone()
    for part, name in OUTPUTS[case.entry].items():
        if name in bufs and not (deferred(case, nz) and part in _PARTIALS[case.entry][2:]):
            v = bufs[name].view().cpu().clone()
            got[part] = v.reshape(-1) if part in ("rowsum", "db") else v
    if case.aux_write:
        got["aux"] = bufs["aux"].view().cpu().clone()
    return got


def memory_violations(case, bufs, nz):
    """-> messages, one per buffer that holds a change where the call may not write: inputs anywhere, outputs outside
    their matrix (padding columns, rows past the end, guard bands), deferred destinations anywhere, ws past the partials"""
    bad = []
    written = set(OUTPUTS[case.entry].values()) | ({"aux"} if case.aux_write else set())
    if deferred(case, nz):
        written -= set(_PARTIALS[case.entry][2:])
    for name, buf in bufs.items():
        if name == "ws":
            rows, cols = split_dims(case)
            used = nz * (rows * cols + rows) if nz > 1 else 0
            if not buf.intact(first=used):
                bad.append(f"ws: changed past its {used} floats of partials (or before its start)")
        elif name in written:
            if not buf.outside_intact():
                bad.append(f"{name}: written outside the {buf.rows} x {buf.cols} matrix (ld {buf.ld})")
        elif not buf.intact():
            bad.append(f"{name}: changed, and the call may only read it")
    return bad
