"""Frechet distance of feature sets (csrc/frechet.hip): float64, forward only, no autograd."""
import ctypes
import math

import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["frechet_state", "frechet_update", "frechet_moments", "f64_gemm", "sym_eig", "frechet_distance", "f64_gemm_ld"]


def _frechet_state_f(who, state):
    """F of a moment state, or ValueError: the contiguous float64 vector (1 + F + F F,) that frechet_state returns"""
    ok = torch.is_tensor(state) and state.dim() == 1 and state.dtype == torch.float64 and state.is_contiguous()
    F = (math.isqrt(max(4 * state.numel() - 3, 0)) - 1) // 2 if ok else 0
    if not ok or 1 + F + F * F != state.numel() or not 1 <= F <= H.FRECHET_MAX_F:
        raise ValueError(f"{who}: the state is {ck.said(state)}; frechet_state gives a contiguous float64 vector (1 + F + F F,), "
                         f"1 <= F <= {H.FRECHET_MAX_F} on the MI355X path")
    return F


def frechet_state(F, device):
    """empty streaming moment state, float64 (1 + F + F F,): n | mean (F) | M2 (F,F), all 0"""
    F = ck.feature_count("frechet_state", F)
    return torch.zeros(1 + F + F * F, dtype=torch.float64, device=device)


def frechet_update(state, feats):
    """fold the rows of feats (n_b, F) into the state: batch mean and centred scatter in double (one tiled SYRK on the
    fp64 MFMA), merged by Chan's rule.  Memory does not grow with the number of rows folded."""
    F = _frechet_state_f("frechet_update", state)
    feats = ck.feature_rows("frechet_update", "feats", feats, least=0, defer=True)
    if feats.shape[1] != F:
        raise ValueError(f"frechet_update: feats has F = {feats.shape[1]} features; the state holds floating (rows, {F})")
    if feats.shape[0] == 0:
        return state
    ck.finite("frechet_update", "feats", feats)
    ws = torch.empty(F, dtype=torch.float64, device=state.device)
    H.call("mmvae_frechet_update", H.ptr(state), H.ptr(feats), H.ptr(ws), feats.shape[0], F, H.stream())
    return state


def frechet_moments(state):
    """-> (n, mu (F,) float64, sigma (F,F) float64 = M2 / (n - 1): np.cov's normalisation, n >= 2)"""
    F = _frechet_state_f("frechet_moments", state)
    n = int(state[0])
    if n < 2:
        raise ValueError(f"frechet_moments: n = {n} rows folded (a covariance needs n >= 2)")
    mu = torch.empty(F, dtype=torch.float64, device=state.device)
    sigma = torch.empty(F, F, dtype=torch.float64, device=state.device)
    H.call("mmvae_frechet_finish", H.ptr(state), H.ptr(mu), H.ptr(sigma), n, F, H.stream())
    return n, mu, sigma


def f64_gemm(A, B, trans_b=False):
    """C = A B (or A B^T) of row-major float64 (F,F) matrices on the fp64 MFMA tile routine"""
    A, B = ck.f64_square("f64_gemm", "A", A), ck.f64_square("f64_gemm", "B", B)
    if A.shape != B.shape:
        raise ValueError(f"f64_gemm: A {tuple(A.shape)} and B {tuple(B.shape)} differ")
    C = torch.empty_like(A)
    H.call("mmvae_f64_gemm", H.ptr(A), H.ptr(B), H.ptr(C), A.shape[0], int(bool(trans_b)), H.stream())
    return C


def sym_eig(S, vectors=True, max_sweeps=H.EIG_MAX_SWEEPS):
    """One-sided Jacobi of the symmetric float64 S (F,F) in round-robin order, one launch per step (include/mmvae_hip.h:
    mmvae_sym_eig) -> {"values": (F,) = |A_j|, the eigenvalues of a positive semi-definite S, unsorted, "vectors": (F,F)
    with column j the eigenvector of values[j] (None for vectors=False: the same values bit for bit), "sweeps": int,
    "rotations": [counted rotations per sweep]}.  The host reads one integer per sweep.  RuntimeError when the sweeps reach
    `max_sweeps` (at most 30) without converging."""
    S = ck.f64_square("sym_eig", "S", S)
    F, max_sweeps = S.shape[0], int(max_sweeps)
    if not 1 <= max_sweeps <= H.EIG_MAX_SWEEPS:
        raise ValueError(f"sym_eig: max_sweeps = {max_sweeps} (1 .. {H.EIG_MAX_SWEEPS})")
    ck.finite("sym_eig", "S", S)
    dev = S.device
    ws = torch.empty(H.lib().mmvae_sym_eig_ws_doubles(F), dtype=torch.float64, device=dev)
    Vc = torch.empty(F, F, dtype=torch.float64, device=dev) if vectors else None
    values = torch.empty(F, dtype=torch.float64, device=dev)
    sweeps, rot = ctypes.c_int(0), (ctypes.c_int * max_sweeps)()
    H.call("mmvae_sym_eig", H.ptr(S), H.ptr(ws), H.ptr(Vc), H.ptr(values), ctypes.byref(sweeps), rot, F, max_sweeps,
           H.stream())
    return {"values": values, "vectors": None if Vc is None else Vc.t(), "sweeps": sweeps.value,
            "rotations": list(rot[:sweeps.value])}


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2 of float64 moments on the device, the square root through two
    symmetric eigendecompositions: (lambda, V) of S1, R = diag(sqrt(lambda)) V^T, G = R S2 R^T, tr (S1 S2)^1/2 = sum_j
    sqrt(sigma_j(G)).  -> {"distance": float64 0-d tensor, "tr_covmean": float64 0-d tensor, "sweeps": (s1, s2)}."""
    sigma1, sigma2 = ck.f64_square("frechet_distance", "sigma1", sigma1), ck.f64_square("frechet_distance", "sigma2", sigma2)
    F = sigma1.shape[0]
    for what, t, shape in (("mu1", mu1, (F,)), ("mu2", mu2, (F,)), ("sigma2", sigma2, (F, F))):
        if tuple(t.shape) != shape or t.dtype != torch.float64:
            raise ValueError(f"frechet_distance: {what} of shape {tuple(t.shape)}, {t.dtype}; float64 {shape} beside sigma1 "
                             f"(1 .. {H.FRECHET_MAX_F} features are on the MI355X path)")
    mu1, mu2 = mu1.contiguous(), mu2.contiguous()
    if not all(bool(torch.isfinite(t).all()) for t in (mu1, mu2, sigma1, sigma2)):
        raise ValueError("frechet_distance: the moments hold values that are not finite")
    dev = sigma1.device
    ws = torch.empty(H.lib().mmvae_frechet_ws_doubles(F), dtype=torch.float64, device=dev)
    out = torch.empty(5, dtype=torch.float64, device=dev)
    sweeps = (ctypes.c_int * 2)()
    H.call("mmvae_frechet_distance", H.ptr(mu1), H.ptr(sigma1), H.ptr(mu2), H.ptr(sigma2), H.ptr(ws), H.ptr(out), sweeps, F,
           H.stream())
    return {"distance": out[0], "tr_covmean": out[1], "sweeps": (sweeps[0], sweeps[1])}


def f64_gemm_ld(A, B, out, trans_b=False, scale=None):
    """out (M,N) <- (A diag(scale)) B, or (A diag(scale)) B^T for trans_b: A (M,K), B (K,N) or (N,K), `out` float64 blocks
    with contiguous rows -- slices of larger row-major matrices are read and written in place, nothing else of `out`'s
    matrix is touched.  `scale` (K,) float64 multiplies the columns of A as they are loaded (None: the plain product).  The
    fp64 MFMA tile routine of f64_gemm; M, N, K need be no multiples of its tile.  `out` must not share memory with A or
    B.  -> out"""
    who = "f64_gemm_ld"
    A, B, out = ck.f64_block(who, "A", A), ck.f64_block(who, "B", B), ck.f64_block(who, "out", out)
    (M, K), (N, Kb) = A.shape, (B.shape if trans_b else B.shape[::-1])
    if Kb != K or tuple(out.shape) != (M, N):
        raise ValueError(f"{who}: A {tuple(A.shape)}, B {tuple(B.shape)} (trans_b = {bool(trans_b)}), out "
                         f"{tuple(out.shape)} do not form a product")
    if scale is not None:
        if not torch.is_tensor(scale) or tuple(scale.shape) != (K,) or scale.dtype != torch.float64:
            raise ValueError(f"{who}: scale must be float64 ({K},), one factor per column of A")
        scale = scale.contiguous()
    store = out.untyped_storage().data_ptr()
    if store in (A.untyped_storage().data_ptr(), B.untyped_storage().data_ptr()):
        raise ValueError(f"{who}: out shares its memory with an operand")
    if not (A.is_cuda and B.is_cuda and out.is_cuda):
        raise ValueError(f"{who}: the blocks are on {A.device}, {B.device}, {out.device}; the kernel runs on the MI355X "
                         f"(there is no host path)")
    H.call("mmvae_f64_gemm_ld", H.ptr(A), A.stride(0), H.ptr(B), B.stride(0), H.ptr(out), out.stride(0), H.ptr(scale), M, N, K,
           int(bool(trans_b)), H.stream())
    return out
