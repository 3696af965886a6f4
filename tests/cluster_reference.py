"""Float64 restatement of the latent cluster analysis: k-means (Lloyd) from given start centres, the
statistics of a partition with the Calinski-Harabasz and Davies-Bouldin indices, the silhouette, and the agreement of two
labelings, as scikit-learn computes them.  Everything is numpy float64 from the fp32 rows with DIRECT differences: no Gram
product, the distance matrices are written out.  Also the seeded inputs of the GPU tests, the margins that make exact
labels a fair demand, and the rounding bars."""
import functools

import numpy as np

U = 2.0 ** -53
SEED = 11
N_INIT = 3
# (N, F, C), each the smallest at which one mechanism can go wrong: less than one tile | a ragged row tile, every cluster
# run padded | F no multiple of 32, uneven sizes | many clusters, a singleton (row 5 is an outlier that restart 0 starts
# from) | the longest feature loop | clusters over several tiles, more than one chunk
SHAPES = ((9, 3, 2), (70, 5, 3), (200, 33, 7), (130, 256, 16), (70, 2048, 4), (1100, 64, 10))
SINGLETON, OUTLIER = 3, 5
# the crafted partition: N = 195, seven ids of which 1 and 5 are unused, 3 and 6 singletons; one row of cluster 0 is a copy of another
CRAFTED_SIZES = (64, 0, 65, 1, 64, 0, 1)
CRAFTED_F = 17


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def features(N, F, C, seed=SEED, labels=None):
    """X = centres[i mod C] + noise (or centres[labels[i]]), fp32: centres standard normal, the noise of deviation
    sqrt(2 F) / 4 -- two centres are four deviations apart on average, whatever F: the clusters overlap a little"""
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((C, F))
    of = np.arange(N) % C if labels is None else np.asarray(labels)
    return (centres[of] + np.sqrt(2.0 * F) / 4.0 * rs.standard_normal((N, F))).astype(np.float32)


def draw(N, C, n_init, seed):
    """rs = RandomState(seed); per restart in order rs.permutation(N)[:C] -> (n_init, C) int32"""
    rs = np.random.RandomState(seed)
    return np.stack([rs.permutation(N)[:C] for _ in range(n_init)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(i):
    """-> (X (N,F) fp32, init (N_INIT, C) int32 row numbers), read-only"""
    N, F, C = SHAPES[i]
    X = features(N, F, C, SEED + i)
    init = draw(N, C, N_INIT, SEED + 100 + i)
    if i == SINGLETON:
        X[OUTLIER] += np.float32(6.0)
        if OUTLIER not in init[0]:
            init[0, 0] = OUTLIER
    X.setflags(write=False)
    init.setflags(write=False)
    return X, init


@functools.lru_cache(maxsize=None)
def crafted():
    """-> (X (195, 17) fp32, labels (195,) int32 with ids 0 .. 6 in a seeded order, other (195,) int32: a second labeling,
    i mod 3, (a, b): row b is a copy of row a, the first two rows of cluster 0)"""
    ids = np.repeat(np.arange(len(CRAFTED_SIZES)), CRAFTED_SIZES)
    labels = ids[np.random.RandomState(SEED + 50).permutation(len(ids))].astype(np.int32)
    X = features(len(labels), CRAFTED_F, len(CRAFTED_SIZES), SEED + 51, labels=labels)
    a, b = (int(i) for i in np.flatnonzero(labels == 0)[:2])
    X[b] = X[a]
    other = (np.arange(len(labels)) % 3).astype(np.int32)
    for t in (X, labels, other):
        t.setflags(write=False)
    return X, labels, other, (a, b)


# ---- k-means -------------------------------------------------------------------------------------------------------------------
def sqdist_to(X64, mu):
    """(N, C): sum_f (x_if - mu_cf)^2 by direct differences"""
    out = np.empty((len(X64), len(mu)))
    for c in range(len(mu)):
        d = X64 - mu[c]
        out[:, c] = (d * d).sum(1)
    return out


def start_centres(X, init):
    init = np.asarray(init)
    return X.astype(np.float64)[init] if init.ndim == 2 else np.array(init, dtype=np.float64)


def kmeans(X, init, max_iter=300):
    """Lloyd's iteration as the contract states it, per restart -> {"labels" (R,N) int32, "centres" (R,C,F), "inertia" (R,),
    "n_iter", "converged", "empty" (R,), "counts" (R,C), "best", and for the fairness assertion "gap": the smallest
    difference between the best and the second-best d^2 over all iterations and rows, "scale": max(|x|^2, |mu|^2) over all
    rows and all centres met, "ever_empty": whether a cluster ever had no rows, "tied": the restarts that share the best
    one's result bit for bit, "best_margin": by how much, relatively, the inertia of every other restart is larger}"""
    X64 = X.astype(np.float64)
    mus = start_centres(X, init)
    R, C, F = mus.shape
    N = len(X64)
    out = {"labels": np.empty((R, N), dtype=np.int32), "centres": np.empty((R, C, F)), "inertia": np.empty(R),
           "n_iter": np.empty(R, dtype=np.int32), "converged": np.empty(R, dtype=bool), "empty": np.zeros(R, dtype=np.int32),
           "counts": np.empty((R, C), dtype=np.int32)}
    gap, scale, ever_empty = np.inf, float((X64 * X64).sum(1).max()), False

    def assign(mu):
        nonlocal gap, scale
        d2 = sqdist_to(X64, mu)
        scale = max(scale, float((mu * mu).sum(1).max()))
        if C > 1:
            two = np.partition(d2, 1, axis=1)
            gap = min(gap, float((two[:, 1] - two[:, 0]).min()))
        return d2.argmin(1).astype(np.int32), d2      # (argmin: the first of equal values)

    for r in range(R):
        mu, prev, converged, t = mus[r].copy(), None, False, 0
        while t < max_iter:
            t += 1
            lab, d2 = assign(mu)
            if prev is not None and np.array_equal(lab, prev):
                converged = True
                break
            for c in range(C):
                rows = X64[lab == c]
                if len(rows):
                    mu[c] = np.add.reduce(rows, axis=0) / len(rows)      # (rows in index order)
                else:
                    out["empty"][r] += 1
                    ever_empty = True
            prev = lab
        if not converged:
            lab, d2 = assign(mu)
        out["labels"][r], out["centres"][r], out["n_iter"][r], out["converged"][r] = lab, mu, t, converged
        out["inertia"][r] = d2[np.arange(N), lab].sum()
        out["counts"][r] = np.bincount(lab, minlength=C)
    best = int(np.argmin(out["inertia"]))      # (the first of equal values)
    # restarts that ended with the best one's centres and labels bit for bit share its sums, here and on the device: their tie
    # goes to the lowest index.  Every other restart must lose by a margin for `best` to be a fair demand.
    tied = [r for r in range(R) if np.array_equal(out["centres"][r], out["centres"][best])
            and np.array_equal(out["labels"][r], out["labels"][best])]
    margin = min([out["inertia"][r] / out["inertia"][best] - 1.0 for r in range(R) if r not in tied], default=np.inf)
    out.update(best=best, tied=tied, best_margin=float(margin), gap=gap, scale=scale, ever_empty=ever_empty)
    return out


def bar(F, scale):
    """the rounding of one squared distance: 8 F 2^-53 max(|x|^2, |mu|^2)"""
    return 8.0 * F * U * scale


@functools.lru_cache(maxsize=None)
def fit(i, max_iter=300):
    X, init = case(i)
    return kmeans(X, init, max_iter)


# ---- statistics of a partition ---------------------------------------------------------------------------------------------------
def stats(X, labels, C):
    """-> {"counts" (C,) int, "means" (C,F) (0 for a cluster without rows), "within" (C,), "wdist" (C,)} and the bounds the
    device is held to.  "tol_element" = 4 F 2^-53 max|x|: the bound on an element of a mean, hence on an element of x - m.
    Carried through the sums: |d within_c| <= sum_{i,f} (2 |x_if - m_cf| + e) e + (n_c + F) 2^-53 within_c, and, a norm
    moving by no more than what is added to its vector, |d wdist_c| <= n_c sqrt(F) e + (n_c + F) 2^-53 wdist_c."""
    X64, labels = X.astype(np.float64), np.asarray(labels)
    F = X64.shape[1]
    e = 4.0 * F * U * float(np.abs(X64).max())
    out = {"counts": np.bincount(labels, minlength=C).astype(np.int64), "means": np.zeros((C, F)), "within": np.zeros(C),
           "wdist": np.zeros(C), "tol_element": e, "tol_within": np.zeros(C), "tol_wdist": np.zeros(C)}
    for c in range(C):
        rows = X64[labels == c]
        if len(rows):
            out["means"][c] = np.add.reduce(rows, axis=0) / len(rows)
            d = rows - out["means"][c]
            d2 = (d * d).sum(1)
            out["within"][c], out["wdist"][c] = d2.sum(), np.sqrt(d2).sum()
            out["tol_within"][c] = ((2.0 * np.abs(d) + e) * e).sum() + (len(rows) + F) * U * out["within"][c]
            out["tol_wdist"][c] = len(rows) * np.sqrt(F) * e + (len(rows) + F) * U * out["wdist"][c]
    return out


def indices(st):
    """(Calinski-Harabasz, Davies-Bouldin) from the statistics, as scikit-learn's calinski_harabasz_score and
    davies_bouldin_score compute them, over the clusters that have rows"""
    on = st["counts"] > 0
    n, m, within, wdist = st["counts"][on].astype(np.float64), st["means"][on], st["within"][on], st["wdist"][on]
    N, C = n.sum(), len(n)
    mean = (n[:, None] * m).sum(0) / N
    extra, intra = float((n * ((m - mean) ** 2).sum(1)).sum()), float(within.sum())
    ch = 1.0 if intra == 0.0 else extra * (N - C) / (intra * (C - 1.0))
    spread = wdist / n
    between = np.sqrt(((m[:, None, :] - m[None, :, :]) ** 2).sum(2))
    if np.allclose(spread, 0) or np.allclose(between, 0):
        return ch, 0.0
    between[between == 0] = np.inf
    db = float(np.mean(np.max((spread[:, None] + spread[None, :]) / between, axis=1)))
    return ch, db


# ---- silhouette -------------------------------------------------------------------------------------------------------------------
def distances(X):
    """(N, N): Euclidean distances by direct differences, an exact 0 on the diagonal"""
    X64 = X.astype(np.float64)
    N, F = X64.shape
    D = np.empty((N, N))
    step = max(1, (1 << 22) // (N * F))
    for i0 in range(0, N, step):
        d = X64[i0:i0 + step, None, :] - X64[None, :, :]
        D[i0:i0 + step] = np.sqrt((d * d).sum(2))
    return D


def silhouette_from_sums(S, labels, counts):
    """the samples from S (N, C) and the counts, float64: a = S[i, l] / (n_l - 1), b = min over the other clusters with rows
    of S[i, c] / n_c, s = (b - a) / max(a, b); 0 in a cluster of one and where max(a, b) = 0 -> (s, a, b, the cluster of b)"""
    S, labels, counts = np.asarray(S, dtype=np.float64), np.asarray(labels), np.asarray(counts)
    N, C = S.shape
    own = counts[labels]
    a = S[np.arange(N), labels] / np.maximum(own - 1, 1)
    other = np.where((counts[None, :] > 0) & (np.arange(C)[None, :] != labels[:, None]), S / np.maximum(counts, 1)[None, :],
                     np.inf)
    near, b = other.argmin(1), other.min(1)
    top = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where((own > 1) & (top > 0), (b - a) / top, 0.0)
    return s, a, b, near


def silhouette(X, labels, C):
    """-> {"sums" S (N,C), "counts", "samples", "score", "tol_sums" (N,C): the bound on the Gram route's error carried
    through the square root, sum_{j in c, j != i} min(sqrt(b), b / d_ij) + N 2^-53 S[i, c] with b = 8 F 2^-53 max |x|^2,
    "tol_samples" (N,): 4 max(tol_a, tol_b) / max(a, b), "sqrt_bar": sqrt(b)}"""
    labels = np.asarray(labels)
    N, F = X.shape
    D = distances(X)
    onehot = (labels[:, None] == np.arange(C)[None, :]).astype(np.float64)
    counts = onehot.sum(0).astype(np.int64)
    assert (counts > 0).sum() >= 2
    S = D @ onehot
    b = 8.0 * F * U * float((X.astype(np.float64) ** 2).sum(1).max())
    with np.errstate(divide="ignore"):
        per = np.minimum(np.sqrt(b), b / D)
    np.fill_diagonal(per, 0.0)
    tol = per @ onehot + N * U * S
    s, a, bb, near = silhouette_from_sums(S, labels, counts)
    tol_a = tol[np.arange(N), labels] / np.maximum(counts[labels] - 1, 1)
    tol_b = tol[np.arange(N), near] / counts[near]
    with np.errstate(divide="ignore", invalid="ignore"):
        tol_s = np.where(np.maximum(a, bb) > 0, 4.0 * np.maximum(tol_a, tol_b) / np.maximum(a, bb), np.inf)
    return {"sums": S, "counts": counts, "samples": s, "score": float(s.mean()), "tol_sums": tol, "tol_samples": tol_s,
            "sqrt_bar": float(np.sqrt(b))}


# ---- agreement of two labelings ---------------------------------------------------------------------------------------------------
def contingency(a, b):
    """T[class of a, cluster of b] over the values that occur, integers"""
    _, ia = np.unique(np.asarray(a), return_inverse=True)
    _, ib = np.unique(np.asarray(b), return_inverse=True)
    T = np.zeros((ia.max() + 1, ib.max() + 1), dtype=np.int64)
    np.add.at(T, (ia, ib), 1)
    return T


def _entropy(n):
    n = n[n > 0].astype(np.float64)
    return float(-np.sum((n / n.sum()) * (np.log(n) - np.log(n.sum()))))


def agreement(a, b):
    """a: the classes, b: the clusters -> {"ari", "nmi", "homogeneity", "completeness", "purity"} as scikit-learn's
    adjusted_rand_score, normalized_mutual_info_score (arithmetic mean) and homogeneity_completeness_v_measure define them"""
    T = contingency(a, b)
    N = int(T.sum())
    ra, rb = T.sum(1), T.sum(0)
    sq = int((T * T).sum())
    tp, fp, fn = sq - N, int((T @ rb).sum()) - sq, int((T.T @ ra).sum()) - sq
    tn = N * N - fp - fn - sq
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    i, j = np.nonzero(T)
    v = T[i, j].astype(np.float64)
    mi = float(max(np.sum(v / N * (np.log(v) - np.log(N)) + v / N * (-np.log(ra[i] * rb[j].astype(np.float64)) + 2 * np.log(N))),
                   0.0))
    ha, hb = _entropy(ra), _entropy(rb)
    if len(ra) == 1 and len(rb) == 1:
        nmi = 1.0
    else:
        nmi = 0.0 if mi <= np.finfo(np.float64).eps else mi / max(0.5 * (ha + hb), np.finfo(np.float64).eps)
    return {"ari": float(ari), "nmi": float(nmi), "homogeneity": mi / ha if ha else 1.0,
            "completeness": mi / hb if hb else 1.0, "purity": float(T.max(0).sum()) / N}


AGREEMENT = ("ari", "nmi", "homogeneity", "completeness", "purity")
