"""Canonical correlation of feature pairs and sentence features (csrc/cca.hip): float64, forward only, no autograd."""
import itertools
import math

import torch

from .. import hipops as H
from . import _checks as ck
from .frechet import f64_gemm_ld, sym_eig

__all__ = ["cca_check_widths", "cca_fit", "cca_score", "sentence_features"]


def cca_check_widths(who, widths, O):
    try:
        widths = [int(w) for w in widths]
    except TypeError:
        raise ValueError(f"{who}: widths = {widths!r} (the feature width of every view, in order)") from None
    if not 2 <= len(widths) <= H.CCA_MAX_VIEWS or min(widths) < 1:
        raise ValueError(f"{who}: widths = {widths} (2 .. {H.CCA_MAX_VIEWS} views of at least one feature each)")
    if sum(widths) != O:
        raise ValueError(f"{who}: widths = {widths} sum to {sum(widths)}, the moments hold O = {O} features")
    if O > H.FRECHET_MAX_F:
        raise ValueError(f"{who}: the views hold O = {O} features side by side; the eigensolver takes at most "
                         f"{H.FRECHET_MAX_F} in all (MMVAE_FRECHET_MAX_F) on the MI355X path: reduce a view's features first")
    return widths


def cca_fit(mu, sigma, widths, k, ridge=1e-12):
    """Multi-view canonical correlation analysis from the moments of the stacked views: the arithmetic of the reference's
    cca (eval/mnistsvhn_helper.py:26-78) in float64 on the device.  `mu` (O,), `sigma` (O,O): frechet_moments of rows that
    hold the views' features side by side, view i `widths[i]` wide, O = sum(widths).  The reference solves A v = lambda B v,
    B = the block diagonal of the views' covariances + ridge I, A = the off-diagonal blocks + ridge I (its quirk, kept).
    Here, with W = B^-1/2 built per view from sym_eig (B_i = Q L Q^T, W_i = Q L^-1/2 Q^T), the symmetric positive
    semi-definite N = W (sigma + 2 ridge I) W has the eigenvalues 1 + lambda and the eigenvectors u, v = W u: sym_eig(N),
    a stable descending sort (ties keep solver order), the k largest.  Every product is f64_gemm_ld on sub-blocks of
    (O,O) matrices; no block-diagonal W is multiplied out.
    -> {"correlations": (k,) float64 = value - 1, "projections": [(o_i, k) float64 per view], the columns of the stacked
        (O, k) matrix scaled to unit Euclidean norm (what scipy.linalg.eig returns; the sign of a column is the solver's),
        "means": [the slices of mu], "sweeps": {"views": [per view], "joint": of N}, "condition": [lambda_min / lambda_max
        of B_i per view], "widths", "k"}.
    2 .. 8 views, O <= 2048, 1 <= k <= min(min(widths), 64), ridge > 0.  A view whose covariance is rank-deficient is
    ill-posed at the default ridge (float64 eig(A, B) itself is): the remedy is the caller's, a ridge near 1e-3 of the
    feature variance.
    Deviations from the reference: k is required (its k=None picks k by an Otsu threshold of scikit-image, not restated);
    the covariances are float64 from the float32 features, where the reference forms them in float32 torch.mm."""
    who = "cca_fit"
    if not torch.is_tensor(sigma) or sigma.dim() != 2 or sigma.shape[0] != sigma.shape[1] or sigma.dtype != torch.float64 \
            or not torch.is_tensor(mu) or tuple(mu.shape) != (sigma.shape[0],) or mu.dtype != torch.float64:
        raise ValueError(f"{who}: mu (O,) and sigma (O,O) are the float64 moments frechet_moments returns")
    O = sigma.shape[0]
    widths = cca_check_widths(who, widths, O)
    k, ridge = int(k), float(ridge)
    if not 1 <= k <= min(min(widths), H.CCA_MAX_K):
        raise ValueError(f"{who}: k = {k} (1 .. min(narrowest view = {min(widths)}, {H.CCA_MAX_K}) on the MI355X path)")
    if not (ridge > 0.0 and math.isfinite(ridge)):
        raise ValueError(f"{who}: ridge = {ridge} (a positive number: B must be positive definite)")
    if not bool(torch.isfinite(sigma).all()) or not bool(torch.isfinite(mu).all()):
        raise ValueError(f"{who}: the moments hold values that are not finite")
    ck.need_gpu(who, "the moments are", sigma.device, "the kernels run")
    dev, mu = sigma.device, mu.contiguous()
    S = sigma.clone(memory_format=torch.contiguous_format)
    S.diagonal().add_(2.0 * ridge)
    offs = [0] + list(itertools.accumulate(widths))
    W = torch.zeros(O, O, dtype=torch.float64, device=dev)
    lows, highs, view_sweeps = [], [], []
    for lo, hi in zip(offs, offs[1:]):
        Bi = sigma[lo:hi, lo:hi].clone(memory_format=torch.contiguous_format)
        Bi.diagonal().add_(ridge)
        e = sym_eig(Bi)
        lam, Q = e["values"], e["vectors"].contiguous()
        lows.append(lam.min())
        highs.append(lam.max())
        view_sweeps.append(e["sweeps"])
        f64_gemm_ld(Q, Q, W[lo:hi, lo:hi], trans_b=True, scale=lam.rsqrt())
    lows, highs = torch.stack(lows).tolist(), torch.stack(highs).tolist()
    if not all(l > 0.0 for l in lows) or not bool(torch.isfinite(W).all()):
        raise ValueError(f"{who}: a view's covariance + ridge I is singular in float64 (smallest eigenvalues {lows}); "
                         f"raise `ridge`")
    T, N = torch.empty_like(W), torch.empty_like(W)
    for lo, hi in zip(offs, offs[1:]):
        f64_gemm_ld(W[lo:hi, lo:hi], S[lo:hi, :], T[lo:hi, :])          # T = W S, a row of blocks per launch
    for lo, hi in zip(offs, offs[1:]):
        f64_gemm_ld(T[:, lo:hi], W[lo:hi, lo:hi], N[:, lo:hi])          # N = T W, a column of blocks per launch
    N = (N + N.t()) * 0.5      # W is symmetric to rounding only; the solver wants the two halves equal
    e = sym_eig(N)
    order = torch.sort(e["values"], descending=True, stable=True).indices[:k]
    U = e["vectors"][:, order].contiguous()
    P = torch.empty(O, k, dtype=torch.float64, device=dev)
    for lo, hi in zip(offs, offs[1:]):
        f64_gemm_ld(W[lo:hi, lo:hi], U[lo:hi, :], P[lo:hi, :])
    P = P / torch.linalg.vector_norm(P, dim=0, keepdim=True)
    return {"correlations": e["values"][order] - 1.0, "projections": [P[lo:hi].contiguous() for lo, hi in zip(offs, offs[1:])],
            "means": [mu[lo:hi].contiguous() for lo, hi in zip(offs, offs[1:])],
            "sweeps": {"views": view_sweeps, "joint": e["sweeps"]}, "condition": [l / h for l, h in zip(lows, highs)],
            "widths": widths, "k": k}


def _cca_side(who, name, x, mean, proj):
    """one view of cca_score -> (contiguous fp32 rows, their finite check left to the caller, mean, proj)"""
    x = ck.rows(who, name, x, 2, "(rows, o) features",
                ((1, 1, H.FRECHET_MAX_F, f"{name} has o = {{1}} features (1 .. {H.FRECHET_MAX_F} are on the MI355X path)"),),
                defer=True)
    o = x.shape[1]
    for what, t, dims in ((f"mean_{name}", mean, 1), (f"proj_{name}", proj, 2)):
        if not torch.is_tensor(t) or t.dim() != dims or t.shape[0] != o or t.dtype != torch.float64:
            raise ValueError(f"{who}: {what} is {ck.said(t)}; float64 ({o},{'' if dims == 1 else ' k'}) beside {name}")
    return x, mean.contiguous(), proj.contiguous()


def cca_score(a, b, mean_a, mean_b, proj_a, proj_b):
    """The cross-modal correlation of paired feature rows a (rows, o_a), b (rows, o_b) under a fit (cca_fit's means and
    projections, float64 (o,) and (o, k)): per row r, p = (a_r - mean_a) proj_a, q = (b_r - mean_b) proj_b and
    cos_r = p . q / (max(|p|, 1e-8) max(|q|, 1e-8)), F.cosine_similarity's clamp.  One kernel: the rows are converted and
    centred in double as they are loaded, both products run on the fp64 MFMA, the projections are never written.
    -> (cos (rows,) float64, their sum, a float64 0-d tensor added in a fixed order: two runs give the same bits)."""
    who = "cca_score"
    a, mean_a, proj_a = _cca_side(who, "a", a, mean_a, proj_a)
    b, mean_b, proj_b = _cca_side(who, "b", b, mean_b, proj_b)
    rows, k = a.shape[0], proj_a.shape[1]
    if b.shape[0] != rows or not 1 <= rows <= H.CCA_MAX_ROWS:
        raise ValueError(f"{who}: a has {rows} rows, b {b.shape[0]} (the same rows of both views, at least one)")
    if proj_b.shape[1] != k or not 1 <= k <= H.CCA_MAX_K:
        raise ValueError(f"{who}: proj_a has k = {k} columns, proj_b {proj_b.shape[1]} (the same 1 .. {H.CCA_MAX_K} on the "
                         f"MI355X path)")
    ck.need_gpu(who, "a is", a.device)
    if not bool(torch.isfinite(a).all() & torch.isfinite(b).all()):      # (one read for both views)
        raise ValueError(f"{who}: the features hold values that are not finite")
    cos = torch.empty(rows, dtype=torch.float64, device=a.device)
    total = torch.empty(1, dtype=torch.float64, device=a.device)
    H.call("mmvae_cca_score", H.ptr(a), H.ptr(b), H.ptr(mean_a), H.ptr(mean_b), H.ptr(proj_a), H.ptr(proj_b), H.ptr(cos),
           H.ptr(total), rows, a.shape[1], b.shape[1], k, H.stream())
    return cos, total[0]


def sentence_features(ids, emb, weights, eos=2, pc=None):
    """Frequency-weighted sentence embeddings, the reference's apply_weights and apply_pc (eval/mnistsvhn_helper.py:165-177):
    ids (B, T) integer tokens, emb (V, E) the embedding table, weights (V,) the tokens' weights (coherence.sif_weights).
    Per sentence L = index of the first `eos` + 1 (T without one), f = (sum_{t < L} weights[id_t] emb[id_t]) / L in double
    in token order; with `pc` (E,) float64, a unit vector, f <- f - pc (pc . f), the common component removed.  One wave per
    sentence, one rounding to fp32.  -> (B, E) fp32.  1 <= E <= 1024, 1 <= T <= 512; every id must lie in [0, V)."""
    who = "sentence_features"
    if not torch.is_tensor(ids) or ids.dim() != 2 or ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
        raise ValueError(f"{who}: ids are integer (B, T) tokens")
    if not torch.is_tensor(emb) or emb.dim() != 2 or not emb.is_floating_point():
        raise ValueError(f"{who}: emb is the floating (V, E) embedding table")
    (B, T), (V, E) = ids.shape, emb.shape
    if not 1 <= E <= H.SENTENCE_MAX_E or not 1 <= T <= H.SENTENCE_MAX_T or B < 1 or V < 1:
        raise ValueError(f"{who}: B = {B} sentences of T = {T} tokens, V = {V} embeddings of E = {E} (1 <= T <= "
                         f"{H.SENTENCE_MAX_T}, 1 <= E <= {H.SENTENCE_MAX_E} are on the MI355X path)")
    if not torch.is_tensor(weights) or tuple(weights.shape) != (V,) or not weights.is_floating_point():
        raise ValueError(f"{who}: weights are floating ({V},), one per embedding")
    if pc is not None and (not torch.is_tensor(pc) or tuple(pc.shape) != (E,) or pc.dtype != torch.float64):
        raise ValueError(f"{who}: pc is a float64 ({E},) unit vector, or None")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= V:
        raise ValueError(f"{who}: ids in [{lo}, {hi}] outside the table's [0, {V})")
    ck.need_gpu(who, "emb is", emb.device)
    dev = emb.device
    ids = ids.detach().to(device=dev, dtype=torch.int32).contiguous()
    emb, weights = H.f32c(emb.detach()), H.f32c(weights.detach().to(dev))
    pc = None if pc is None else pc.detach().to(dev).contiguous()
    out = torch.empty(B, E, dtype=torch.float32, device=dev)
    H.call("mmvae_sentence_features", H.ptr(ids), H.ptr(emb), H.ptr(weights), H.ptr(pc), H.ptr(out), B, T, E, V, int(eos),
           H.stream())
    return out
