"""Float64 restatement of the latent density estimation: EM for a mixture of Gaussians from start
labels with scikit-learn's GaussianMixture arithmetic (full and diagonal covariances), the scoring of rows, the draws, BIC and
AIC.  Everything is numpy float64 from the fp32 rows, with numpy's own summation order (dot products, pairwise sums), one
restart at a time.  Also the seeded cases of the tests, the facts that make exact iteration counts and labels a fair demand
(no iteration on the knife edge of `tol`, no row between two components), and the tolerance of every compared quantity: the
spread of the restatement itself between the rows in order and a fixed permutation of them."""
import functools

import numpy as np

U = 2.0 ** -53
SEED = 29
REG, TOL, MAX_ITER = 1e-6, 1e-3, 100
# (N, D, C), each the smallest at which one mechanism can go wrong: one row, one component | a block less one row, D = 1 |
# exactly one block | a block and one row, odd D | two blocks and a ragged third, D past half the limit and no multiple of
# 8 | D at the limit | C at the limit, many blocks | more than one 1024-row covariance chunk
SHAPES = ((1, 2, 1), (63, 1, 2), (64, 2, 3), (65, 7, 3), (130, 33, 2), (300, 64, 3), (640, 2, 64), (1100, 7, 3))
EMPTY = len(SHAPES)      # the case after them: (130, 7, 4) with a start that leaves component 2 without rows
# the cases the restatement is held to scikit-learn on
SKLEARN_SHAPES = ((130, 7, 3), (65, 2, 2), (200, 32, 4), (300, 64, 3), (64, 1, 2))
KINDS = ("full", "diag")


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def blobs(N, D, C, seed, ids=None):
    """C centres 3 N(0, 1), rows = centre + N(0, 1) rounded through fp32, start labels = the true labels with 20 % moved to
    the next id (of `ids`, the component ids in use: default 0 .. C - 1) -> (X (N,D) fp32, start (N,) int32, truth (N,))"""
    rs = np.random.RandomState(seed)
    ids = np.arange(C) if ids is None else np.asarray(ids)
    centres = 3.0 * rs.standard_normal((len(ids), D))
    of = np.arange(N) % len(ids)
    X = (centres[of] + rs.standard_normal((N, D))).astype(np.float32)
    moved = rs.random_sample(N) < 0.2
    start = np.where(moved, (of + 1) % len(ids), of)
    return X, ids[start].astype(np.int32), ids[of].astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(i):
    """-> (X (N,D) fp32, start (N,) int32, C), read-only"""
    if i == EMPTY:
        X, start, _ = blobs(130, 7, 3, SEED + 50, ids=(0, 1, 3))
        C = 4
    else:
        N, D, C = SHAPES[i]
        X, start, _ = blobs(N, D, C, SEED + i)
    X.setflags(write=False)
    start.setflags(write=False)
    return X, start, C


def case_ids():
    return [f"{n}x{d}x{c}" for n, d, c in SHAPES] + ["empty-start"]


# ---- EM ------------------------------------------------------------------------------------------------------------------------
class Degenerate(Exception):
    pass


def m_step(X, resp, kind, reg):
    """scikit-learn's _estimate_gaussian_parameters + the weights -> (weights, means, covariances)"""
    N, D = X.shape
    nk = resp.sum(0) + 10.0 * np.finfo(np.float64).eps
    means = resp.T @ X / nk[:, None]
    if kind == "full":
        cov = np.empty((len(nk), D, D))
        for k in range(len(nk)):
            diff = X - means[k]
            cov[k] = (resp[:, k] * diff.T) @ diff / nk[k]
            cov[k].flat[::D + 1] += reg
    else:
        cov = resp.T @ (X * X) / nk[:, None] - means ** 2 + reg
    w = nk / N
    return w / w.sum(), means, cov


def factors(cov, kind):
    """-> (lower Cholesky factors L, precision factors P = L^-T, sum_d log P[d, d]); diag: (sqrt, 1 / sqrt, ...)"""
    if kind == "diag":
        if np.any(~(cov > 0.0)) or not np.all(np.isfinite(cov)):
            raise Degenerate
        L = np.sqrt(cov)
        P = 1.0 / L
        return L, P, np.log(P).sum(1)
    L, P = np.empty_like(cov), np.empty_like(cov)
    for k in range(len(cov)):
        try:
            if not np.all(np.isfinite(cov[k])):
                raise np.linalg.LinAlgError
            L[k] = np.linalg.cholesky(cov[k])
        except np.linalg.LinAlgError:
            raise Degenerate
        if not np.all(np.isfinite(L[k])) or np.any(np.diagonal(L[k]) <= 0.0):
            raise Degenerate
        D = cov.shape[1]
        inv = np.zeros((D, D))
        for j in range(D):      # forward substitution, column by column
            inv[j, j] = 1.0 / L[k, j, j]
            for i in range(j + 1, D):
                inv[i, j] = -(L[k, i, j:i] @ inv[j:i, j]) / L[k, i, i]
        P[k] = inv.T
    return L, P, np.log(np.diagonal(P, axis1=1, axis2=2)).sum(1)


def e_step(X, w, means, P, logdet, kind):
    """-> (norm (N,), log p (N,C) weighted, resp (N,C))"""
    N, D = X.shape
    lp = np.empty((N, len(w)))
    for k in range(len(w)):
        y = (X - means[k]) @ P[k] if kind == "full" else (X - means[k]) * P[k]
        lp[:, k] = -0.5 * (D * np.log(2.0 * np.pi) + (y * y).sum(1)) + logdet[k]
    with np.errstate(divide="ignore"):
        lp = lp + np.log(w)
    top = lp.max(1)
    norm = np.log(np.exp(lp - top[:, None]).sum(1)) + top
    return norm, lp, np.exp(lp - norm[:, None])


def em(X, start, C, kind, reg=REG, tol=TOL, max_iter=MAX_ITER):
    """one restart -> dict; "degenerate": a covariance without a Cholesky factor (then the bound is -inf and nothing else is
    meaningful).  "changes": |lb_t - lb_{t-1}| per iteration; "gap": the smallest difference between a row's two largest
    final responsibilities (1 for one component)."""
    X = np.asarray(X, np.float64)
    N, D = X.shape
    resp = np.zeros((N, C))
    resp[np.arange(N), start] = 1.0
    out = {"degenerate": False, "lower_bound": -np.inf, "n_iter": 0, "converged": False, "changes": []}
    try:
        w, means, cov = m_step(X, resp, kind, reg)
        L, P, logdet = factors(cov, kind)
        lb = -np.inf
        for t in range(1, max_iter + 1):
            out["n_iter"] = t
            norm, _, resp = e_step(X, w, means, P, logdet, kind)
            w, means, cov = m_step(X, resp, kind, reg)
            L, P, logdet = factors(cov, kind)
            prev, lb = lb, norm.mean()
            out["changes"].append(abs(lb - prev))
            if abs(lb - prev) < tol:
                out["converged"] = True
                break
    except Degenerate:
        out["degenerate"] = True
        return out
    norm, lp, resp = e_step(X, w, means, P, logdet, kind)
    top2 = np.sort(resp, 1)[:, -2:] if C > 1 else np.stack([np.zeros(N), np.ones(N)], 1)
    out.update({"weights": w, "means": means, "covariances": cov, "cholesky": L, "precisions_cholesky": P, "log_det": logdet,
                "lower_bound": lb, "labels": lp.argmax(1).astype(np.int32), "resp": resp, "log_density": norm,
                "gap": float((top2[:, 1] - top2[:, 0]).min())})
    return out


def score(X, fit, kind):
    """-> (log-density (N,), labels, resp) of any rows under a fit's parameters"""
    norm, lp, resp = e_step(np.asarray(X, np.float64), fit["weights"], fit["means"], fit["precisions_cholesky"], fit["log_det"],
                            kind)
    return norm, lp.argmax(1).astype(np.int32), resp


def sample(fit, kind, u, eps):
    """-> (z (n,D) float64 = mu_k + L_k eps, components (n,)): the first k with u < w_0 + .. + w_k, the last takes the rest"""
    cum = np.cumsum(fit["weights"])
    comp = np.minimum((np.asarray(u)[:, None] >= cum[None, :]).sum(1), len(cum) - 1)
    eps = np.asarray(eps, np.float64)
    if kind == "full":
        z = fit["means"][comp] + np.einsum("nij,nj->ni", fit["cholesky"][comp], eps)
    else:
        z = fit["means"][comp] + fit["cholesky"][comp] * eps
    return z, comp.astype(np.int32)


def information(C, D, kind, mean_log_density, N):
    n_par = (2 * C * D if kind == "diag" else C * D * (D + 1) // 2 + C * D) + C - 1
    return {"n_parameters": n_par, "bic": -2.0 * mean_log_density * N + n_par * np.log(N),
            "aic": -2.0 * mean_log_density * N + 2 * n_par}


# ---- the shared fits and their tolerances --------------------------------------------------------------------------------------
COMPARED = ("lower_bound", "weights", "means", "covariances", "log_density")


@functools.lru_cache(maxsize=None)
def fit(i, kind):
    """the restatement of case i, read-only, with "tol": {quantity: allowed |difference|} -- the larger of 100 x the spread of
    that quantity between the rows in order and a fixed permutation of them, and 64 ulp of its largest magnitude"""
    X, start, C = case(i)
    ref = em(X, start, C, kind)
    assert not ref["degenerate"]
    perm = np.random.RandomState(SEED + 1000 + i).permutation(len(X))
    other = em(X[perm], start[perm], C, kind)
    assert not other["degenerate"] and other["n_iter"] == ref["n_iter"] and other["converged"] == ref["converged"]
    back = np.empty_like(perm)
    back[perm] = np.arange(len(perm))
    other["log_density"] = other["log_density"][back]
    ref["spread"], ref["tol"] = {}, {}
    for k in COMPARED:
        a, b = np.asarray(ref[k], np.float64), np.asarray(other[k], np.float64)
        ref["spread"][k] = float(np.abs(a - b).max())
        ref["tol"][k] = max(100.0 * ref["spread"][k], 64.0 * np.spacing(float(np.abs(a).max())))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def knife_edge(ref, tol=TOL):
    """the smallest distance of an iteration's |change| from tol, as a share of tol"""
    return min(abs(c - tol) / tol for c in ref["changes"]) if ref["changes"] else np.inf
