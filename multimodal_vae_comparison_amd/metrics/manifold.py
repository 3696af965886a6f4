"""k-nearest-neighbour manifold estimates of feature sets (csrc/manifold.hip): float64 distances, forward only."""
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["manifold_sqnorms", "manifold_radii", "manifold_cross", "manifold_prdc"]


def _manifold_k(who, k):
    k = int(k)
    if not 1 <= k <= H.MANIFOLD_MAX_K:
        raise ValueError(f"{who}: k = {k} neighbours (1 .. {H.MANIFOLD_MAX_K} are on the MI355X path)")
    return k


def _manifold_rows(who, what, X, least=1):
    return ck.feature_rows(who, what, X, least, H.MANIFOLD_MAX_ROWS, f"{least} .. {H.MANIFOLD_MAX_ROWS} are on the MI355X "
                                                                       f"path; the k-th neighbour needs k + 1 rows")


def _manifold_sqnorms(X):
    n2 = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
    H.call("mmvae_manifold_sqnorms", H.ptr(X), H.ptr(n2), X.shape[0], X.shape[1], H.stream())
    return n2


def _manifold_radii(X, n2, k, chunks):
    N, F = X.shape
    ws = torch.empty(H.lib().mmvae_manifold_ws_doubles(N, N, k, chunks), dtype=torch.float64, device=X.device)
    rad2 = torch.empty(N, dtype=torch.float64, device=X.device)
    H.call("mmvae_manifold_radii", H.ptr(X), H.ptr(n2), H.ptr(ws), H.ptr(rad2), N, F, k, chunks, H.stream())
    return rad2


def _manifold_cross(B, nb, A, na, rad2, chunks):
    (Nb, F), Na = B.shape, A.shape[0]
    ws = torch.empty(H.lib().mmvae_manifold_ws_doubles(Nb, Na, 1, chunks), dtype=torch.float64, device=B.device)
    count = torch.empty(Nb, dtype=torch.int32, device=B.device)
    mind2 = torch.empty(Nb, dtype=torch.float64, device=B.device)
    H.call("mmvae_manifold_cross", H.ptr(B), H.ptr(nb), H.ptr(A), H.ptr(na), H.ptr(rad2), H.ptr(ws), H.ptr(count),
           H.ptr(mind2), Nb, Na, F, chunks, H.stream())
    return count, mind2


def manifold_sqnorms(X):
    """-> (N,) float64: |x_i|^2 of the fp32 rows, summed in double in feature order"""
    return _manifold_sqnorms(_manifold_rows("manifold_sqnorms", "X", X))


def manifold_radii(X, k, chunks=0):
    """-> (N,) float64: rad^2[i] = the k-th smallest squared distance from row i of X (N,F) to the other rows, the row itself
    left out by index (a duplicate row is a neighbour at distance 0).  d^2 = max(0, (|x|^2 + |y|^2) - 2 x . y) in double, the
    Gram product on the fp64 MFMA; the N x N matrix is never written.  `chunks`: how many workgroups share a row's columns
    (0: the default plan); the result does not depend on it, bit for bit."""
    k, chunks = _manifold_k("manifold_radii", k), ck.chunks("manifold_radii", chunks)
    X = _manifold_rows("manifold_radii", "X", X, least=k + 1)
    return _manifold_radii(X, _manifold_sqnorms(X), k, chunks)


def _manifold_rad2(who, rad2, A):
    if not torch.is_tensor(rad2) or tuple(rad2.shape) != (A.shape[0],) or rad2.dtype != torch.float64:
        raise ValueError(f"{who}: rad2 is {ck.said(rad2)}; float64 ({A.shape[0]},), one squared radius per manifold row")
    ck.same_device(who, "rad2 is", rad2, "the manifold rows", A)
    rad2 = rad2.detach().contiguous()
    if bool(torch.isnan(rad2).any()):
        raise ValueError(f"{who}: rad2 holds NaN")
    return rad2


def manifold_cross(queries, manifold, rad2, chunks=0):
    """query rows (Nq,F) against manifold rows (Na,F) with their squared radii rad2 (Na,) float64
    -> (count (Nq,) int32 = the number of manifold rows whose sphere holds the query, d^2 <= rad^2: a point on a sphere is
        inside; mind2 (Nq,) float64 = the query's smallest squared distance to the manifold rows)."""
    chunks = ck.chunks("manifold_cross", chunks)
    B = _manifold_rows("manifold_cross", "queries", queries)
    A = _manifold_rows("manifold_cross", "manifold", manifold)
    ck.same_features("manifold_cross", "queries have", B, "the manifold", A)
    ck.same_device("manifold_cross", "the queries are", B, "the manifold rows", A)
    rad2 = _manifold_rad2("manifold_cross", rad2, A)
    return _manifold_cross(B, _manifold_sqnorms(B), A, _manifold_sqnorms(A), rad2, chunks)


def manifold_prdc(real, fake, k=5, chunks=0):
    """Improved precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) of generated
    feature rows `fake` (M,F) against `real` (N,F), k-nearest-neighbour spheres, `<=` throughout:
      rad2_real, rad2_fake   manifold_radii of each set;
      hit_real[j]  = #{i : d^2(fake_j, real_i) <= rad2_real[i]},  hit_fake[i] = #{j : d^2(real_i, fake_j) <= rad2_fake[j]},
      near_real[i] = min_j d^2(real_i, fake_j);
      precision = mean_j [hit_real[j] > 0], recall = mean_i [hit_fake[i] > 0], density = sum_j hit_real[j] / (k M),
      coverage = mean_i [near_real[i] <= rad2_real[i]].
    -> the four as floats (quotients of integer sums: exact counts) and the five per-row tensors on the device."""
    k, chunks = _manifold_k("manifold_prdc", k), ck.chunks("manifold_prdc", chunks)
    R = _manifold_rows("manifold_prdc", "real", real, least=k + 1)
    G = _manifold_rows("manifold_prdc", "fake", fake, least=k + 1)
    ck.same_features("manifold_prdc", "real has", R, "fake", G)
    ck.same_device("manifold_prdc", "real is", R, "fake", G)
    nr, ng = _manifold_sqnorms(R), _manifold_sqnorms(G)
    rad_r, rad_g = _manifold_radii(R, nr, k, chunks), _manifold_radii(G, ng, k, chunks)
    hit_r, _ = _manifold_cross(G, ng, R, nr, rad_r, chunks)
    hit_g, near_r = _manifold_cross(R, nr, G, ng, rad_g, chunks)
    N, M = R.shape[0], G.shape[0]
    return {"precision": int((hit_r > 0).sum()) / M, "recall": int((hit_g > 0).sum()) / N,
            "density": int(hit_r.sum(dtype=torch.int64)) / (k * M), "coverage": int((near_r <= rad_r).sum()) / N,
            "hit_real": hit_r, "hit_fake": hit_g, "near_real": near_r, "rad2_real": rad_r, "rad2_fake": rad_g}
