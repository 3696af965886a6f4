"""Latent cluster analysis (csrc/cluster.hip): k-means, partition statistics, silhouette; float64, forward only."""
import math

import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck
from .manifold import _manifold_sqnorms

__all__ = ["KMEANS_CHECK_EVERY", "kmeans_draw", "kmeans_check_init", "kmeans_fit", "cluster_stats", "cluster_indices",
           "silhouette_plan", "silhouette", "cluster_agreement"]


KMEANS_CHECK_EVERY = 8      # iterations per enqueued call and between two looks at the restarts' states


def _cluster_rows(who, X):
    return ck.feature_rows(who, "X", X, 1, H.MANIFOLD_MAX_ROWS, f"1 .. {H.MANIFOLD_MAX_ROWS} are on the MI355X path")


def _cluster_count(who, C, N):
    C = int(C)
    if not 1 <= C <= H.CLUSTER_MAX_K:
        raise ValueError(f"{who}: {C} clusters (1 .. {H.CLUSTER_MAX_K} are on the MI355X path)")
    if C > N:
        raise ValueError(f"{who}: {C} clusters for {N} rows (at most one cluster per row on the MI355X path)")
    return C


def _cluster_labels(who, what, labels, N, device=None):
    """an integer (N,) tensor (N None: of any length >= 1) of ids >= 0 (on `device`, where one is given) or ValueError
    -> (labels, the largest id)"""
    entries = () if N is None else ((0, N, N, f"{what} has {{0}} entries for {N} rows"),)
    labels = ck.integers(who, what, labels, 1, "an integer (N,) tensor, one cluster id per row", entries, device, "the rows",
                         arrays=(np.ndarray, list, tuple), nonempty=True, to=None)
    lo, hi = ck.extremes(labels)
    if lo < 0:
        raise ValueError(f"{who}: {what} holds negative ids (clusters are numbered from 0)")
    return labels, hi


def _cluster_partition(who, X, labels, n_clusters):
    """the checks shared by cluster_stats and silhouette -> (X fp32, labels int32 on its device, C)"""
    X = _cluster_rows(who, X)
    labels, hi = _cluster_labels(who, "labels", labels, X.shape[0], X.device)
    C = hi + 1 if n_clusters is None else int(n_clusters)
    if not 1 <= C <= H.CLUSTER_MAX_K:
        raise ValueError(f"{who}: {C} clusters (1 .. {H.CLUSTER_MAX_K} are on the MI355X path)")
    if hi >= C:
        raise ValueError(f"{who}: labels holds the id {hi}; n_clusters = {C} has the ids 0 .. {C - 1}")
    return X, labels.to(torch.int32).contiguous(), C


def kmeans_draw(N, C, n_init, seed):
    """the start centres of a k-means fit, drawn on the host: rs = numpy.random.RandomState(seed); per restart, in order,
    rs.permutation(N)[:C] -> (n_init, C) int32 row numbers, no row twice within a restart"""
    rs = np.random.RandomState(seed)
    return np.stack([rs.permutation(N)[:C] for _ in range(n_init)]).astype(np.int32)


def _cluster_spread(labels, d2, C):
    R, N = labels.shape
    counts = torch.empty(R, C, dtype=torch.int32, device=labels.device)
    within, wdist = (torch.empty(R, C, dtype=torch.float64, device=labels.device) for _ in range(2))
    inertia = torch.empty(R, dtype=torch.float64, device=labels.device)
    H.call("mmvae_cluster_spread", H.ptr(labels), H.ptr(d2), H.ptr(counts), H.ptr(within), H.ptr(wdist), H.ptr(inertia), N, C,
           R, H.stream())
    return counts, within, wdist, inertia


def kmeans_check_init(who, init, N, F, C=None):
    """the start centres of a k-means fit on (N, F) rows or ValueError: integer (R, C) row numbers inside [0, N), none twice
    within a restart, or finite float64 (R, C, F) centres; R, C inside the limits, C <= N (and equal to `C`, where given)
    -> (init as a tensor, whether it holds row numbers)"""
    if isinstance(init, np.ndarray):
        init = torch.from_numpy(np.ascontiguousarray(init))
    rows = torch.is_tensor(init) and init.dim() == 2 and not init.is_floating_point() and not init.is_complex() and \
        init.dtype != torch.bool
    if not rows and not (torch.is_tensor(init) and init.dim() == 3 and init.dtype == torch.float64):
        raise ValueError(f"{who}: init is {ck.said(init)}; integer (R, C) row numbers or float64 (R, C, F) centres")
    if not 1 <= init.shape[0] <= H.CLUSTER_MAX_INIT:
        raise ValueError(f"{who}: {init.shape[0]} restarts (1 .. {H.CLUSTER_MAX_INIT} are on the MI355X path)")
    if _cluster_count(who, init.shape[1], N) != (init.shape[1] if C is None else C):
        raise ValueError(f"{who}: init holds {init.shape[1]} centres per restart, n_clusters = {C}")
    init = init.detach()
    if rows:
        lo, hi = ck.extremes(init)
        if lo < 0 or hi >= N:
            raise ValueError(f"{who}: init holds row numbers from {lo} to {hi}; X has the rows 0 .. {N - 1}")
        ordered = torch.sort(init.long(), dim=1).values
        if bool((ordered[:, 1:] == ordered[:, :-1]).any()):
            raise ValueError(f"{who}: init names a row twice within one restart (two equal start centres)")
    else:
        if init.shape[2] != F:
            raise ValueError(f"{who}: init has centres of {init.shape[2]} features, X F = {F}")
        ck.finite(who, "init", init)
    return init, rows


def kmeans_fit(X, init, max_iter=300):
    """k-means (Lloyd) on the rows of X (N,F), read as double, from given start centres, R restarts side by side.
    `init`: integer (R,C) row numbers (centre c of restart r starts as row init[r, c]; kmeans_draw) or float64 (R,C,F)
    centres.  Per restart, iteration t = 1, 2, ...: labels = the nearest centre by d^2 = sum_f (x_f - mu_f)^2 (a tie goes
    to the lowest index); t > 1 and no label changed: converged, n_iter = t; else every centre becomes the mean of its rows
    (summed in index order; a cluster without rows keeps its centre and counts in `empty`); after `max_iter` updates
    without convergence one more assignment gives the labels of the returned centres.  This is scikit-learn's
    KMeans(init=<array>, n_init=1, tol=0, algorithm="lloyd") on float64 input, except that it relocates empty clusters.
    Two launches per iteration for all restarts; the host reads the restarts' states every KMEANS_CHECK_EVERY iterations.
    -> {"centres" (R,C,F) float64, "labels" (R,N) int32, "inertia" (R,) float64 = sum_i d^2[i, label_i], "n_iter" (R,) int32,
        "converged" (R,) bool, "empty" (R,) int32, "counts" (R,C) int32, "best": the restart of the smallest inertia (the
        lowest of equals)}.  Two runs, and a restart alone or beside others, give the same bits."""
    who = "kmeans_fit"
    X = _cluster_rows(who, X)
    N, F = X.shape
    max_iter = int(max_iter)
    if not 1 <= max_iter <= H.CLUSTER_MAX_ITER:
        raise ValueError(f"{who}: max_iter = {max_iter} (1 .. {H.CLUSTER_MAX_ITER} are on the MI355X path)")
    init, rows = kmeans_check_init(who, init, N, F)
    R, C = init.shape[:2]
    init = init.to(X.device)
    ck.need_gpu(who, "X is", X.device, "the kernels run")
    centres = (X.double()[init.long()] if rows else init.clone()).contiguous()
    labels = torch.zeros(R, N, dtype=torch.int32, device=X.device)
    ws = torch.zeros(H.lib().mmvae_cluster_lloyd_ws_ints(N, R), dtype=torch.int32, device=X.device)
    state = ws[:4 * R].view(R, 4)
    for it0 in range(1, max_iter + 1, KMEANS_CHECK_EVERY):
        H.call("mmvae_cluster_lloyd", H.ptr(X), H.ptr(centres), H.ptr(labels), H.ptr(ws), N, F, C, R, it0,
               min(KMEANS_CHECK_EVERY, max_iter - it0 + 1), max_iter, H.stream())
        if bool((state[:, 0] != 0).all()):
            break
    d2 = torch.empty(R, N, dtype=torch.float64, device=X.device)
    H.call("mmvae_cluster_assign", H.ptr(X), H.ptr(centres), H.ptr(labels), H.ptr(d2), N, F, C, R, 0, H.stream())
    counts, _, _, inertia = _cluster_spread(labels, d2, C)
    state = state.clone()
    finished = state[:, 0] != 0
    empties = ws[ws.numel() - R * H.CLUSTER_MAX_K:].view(R, H.CLUSTER_MAX_K)      # (per cluster: the updates it had no rows at)
    return {"centres": centres, "labels": labels, "inertia": inertia,
            "n_iter": torch.where(finished, state[:, 1], torch.full_like(state[:, 1], max_iter)),
            "converged": finished & (state[:, 2] != 0), "empty": empties.sum(1).to(torch.int32), "counts": counts,
            "best": int(np.argmin(inertia.cpu().numpy()))}


def cluster_stats(X, labels, n_clusters):
    """The statistics of the partition `labels` (N,) of the rows of X (N,F) into the ids 0 .. n_clusters - 1, in double:
    -> {"counts" (C,) int32, "means" (C,F) float64 (the rows summed in index order; 0 for an id without rows), "within" (C,)
        = sum_{i in c} |x_i - m_c|^2, "wdist" (C,) = sum_{i in c} |x_i - m_c|, rows in index order}."""
    who = "cluster_stats"
    if n_clusters is None:
        raise ValueError(f"{who}: n_clusters is None (1 .. {H.CLUSTER_MAX_K} are on the MI355X path)")
    X, labels, C = _cluster_partition(who, X, labels, n_clusters)
    ck.need_gpu(who, "X is", X.device, "the kernels run")
    N, F = X.shape
    labels = labels.view(1, N)
    means = torch.zeros(1, C, F, dtype=torch.float64, device=X.device)
    counts = torch.empty(1, C, dtype=torch.int32, device=X.device)
    d2 = torch.empty(1, N, dtype=torch.float64, device=X.device)
    H.call("mmvae_cluster_means", H.ptr(X), H.ptr(labels), H.ptr(means), H.ptr(counts), N, F, C, 1, H.stream())
    H.call("mmvae_cluster_assign", H.ptr(X), H.ptr(means), H.ptr(labels), H.ptr(d2), N, F, C, 1, 1, H.stream())
    counts, within, wdist, _ = _cluster_spread(labels, d2, C)
    return {"counts": counts[0], "means": means[0], "within": within[0], "wdist": wdist[0]}


def cluster_indices(stats):
    """Calinski-Harabasz and Davies-Bouldin indices from cluster_stats' result, on the host in float64 as scikit-learn's
    calinski_harabasz_score and davies_bouldin_score compute them, over the C' clusters that have rows:
      CH = [sum_c n_c |m_c - m|^2 / (C' - 1)] / [sum_c within_c / (N - C')], m the mean of all rows (1 where the clusters
      have no spread); DB = mean_c max_{c' != c} (wdist_c / n_c + wdist_c' / n_c') / |m_c - m_c'| (0 where every spread or
      every distance between means vanishes).  -> {"calinski_harabasz": float, "davies_bouldin": float}"""
    who = "cluster_indices"
    if not isinstance(stats, dict) or any(k not in stats for k in ("counts", "means", "within", "wdist")):
        raise ValueError(f"{who}: stats is what cluster_stats returns (counts, means, within, wdist)")
    n_all, m, within, wdist = (np.asarray(torch.as_tensor(stats[k]).detach().cpu().numpy())
                               for k in ("counts", "means", "within", "wdist"))
    if m.ndim != 2 or any(v.shape != (m.shape[0],) for v in (n_all, within, wdist)):
        raise ValueError(f"{who}: stats holds counts, within, wdist (C,) and means (C, F)")
    on = n_all > 0
    n, m, within, wdist = n_all[on].astype(np.float64), m[on].astype(np.float64), within[on], wdist[on]
    N, C = n.sum(), len(n)
    if not 2 <= C < N:
        raise ValueError(f"{who}: {C} clusters with rows for {int(N)} rows (the indices need 2 .. N - 1)")
    mean = (n[:, None] * m).sum(0) / N
    extra, intra = float((n * ((m - mean) ** 2).sum(1)).sum()), float(within.sum())
    ch = 1.0 if intra == 0.0 else extra * (N - C) / (intra * (C - 1.0))
    spread = wdist / n
    between = np.sqrt(((m[:, None, :] - m[None, :, :]) ** 2).sum(2))
    if np.allclose(spread, 0) or np.allclose(between, 0):
        db = 0.0
    else:
        between[between == 0] = np.inf
        db = float(np.mean(np.max((spread[:, None] + spread[None, :]) / between, axis=1)))
    return {"calinski_harabasz": float(ch), "davies_bouldin": db}


def silhouette_plan(counts, N, chunks):
    """the padded column list's layout and the chunk table from the clusters' sizes (host) -> (tile offset per cluster,
    padded length, table (chunks, 3) int32 = (cluster, first tile, tile past the last), first (C + 1,) int32)"""
    tiles = (counts + 63) // 64
    offset = np.concatenate(([0], np.cumsum(tiles)))
    per = H.lib().mmvae_cluster_sil_tiles_per_chunk(N, int(offset[-1]), chunks)
    table, first = [], [0]
    for c, t in enumerate(tiles):
        table += [(c, int(offset[c]) + t0, int(offset[c]) + min(t0 + per, int(t))) for t0 in range(0, int(t), per)]
        first.append(len(table))
    return offset, 64 * int(offset[-1]), np.array(table, dtype=np.int32).reshape(-1, 3), np.array(first, dtype=np.int32)


def silhouette(X, labels, n_clusters=None, chunks=0):
    """Silhouette of the partition `labels` (N,) of the rows of X (N,F); ids 0 .. n_clusters - 1 (None: the largest id + 1),
    ids without rows allowed.  d(i, j) = sqrt(max(0, (|x_i|^2 + |x_j|^2) - 2 x_i . x_j)) in double, the product on the fp64
    MFMA; S[i, c] = sum_{j in c, j != i} d(i, j), the row itself left out by INDEX (a duplicate row is an ordinary member
    at distance 0); a = S[i, l_i] / (n_l - 1), b = min over the other clusters with rows of S[i, c] / n_c,
    s_i = (b - a) / max(a, b), 0 in a cluster of one row and where max(a, b) = 0.  Neither the N x N matrix nor an N x n_c
    block is written: the columns are walked through a list of row numbers sorted by cluster.  `chunks`: 0 = the default
    plan, or the number of chunks the column list is cut into before the cuts at the cluster borders; two plans regroup
    fp64 sums (agreement to rounding), two runs with one plan give the same bits.
    -> {"samples" (N,) float64, "score": float = mean_i s_i, "sums" S (N,C) float64, "counts" (C,) int64}."""
    who = "silhouette"
    X, labels, C = _cluster_partition(who, X, labels, n_clusters)
    chunks = ck.chunks(who, chunks)
    N, F = X.shape
    lab = labels.long()
    cnt = torch.bincount(lab, minlength=C)
    counts = cnt.cpu().numpy()
    if int((counts > 0).sum()) < 2:
        raise ValueError(f"{who}: labels puts every row into one cluster (the silhouette needs two clusters with rows)")
    ck.need_gpu(who, "X is", X.device, "the kernels run")
    dev = X.device
    offset, padded, table, first = silhouette_plan(counts, N, chunks)
    order = torch.argsort(lab, stable=True)
    of = lab[order]
    start = torch.from_numpy(np.concatenate(([0], np.cumsum(counts)[:-1]))).to(dev)
    place = 64 * torch.from_numpy(offset[:-1]).to(dev)[of] + (torch.arange(N, device=dev) - start[of])
    column_list = torch.full((padded,), -1, dtype=torch.int32, device=dev)
    column_list[place] = order.to(torch.int32)
    n_chunks = len(table)
    ws = torch.empty(H.lib().mmvae_cluster_sil_ws_doubles(N, n_chunks), dtype=torch.float64, device=dev)
    S = torch.empty(N, C, dtype=torch.float64, device=dev)
    n2, table, first = _manifold_sqnorms(X), torch.from_numpy(table).to(dev), torch.from_numpy(first).to(dev)
    H.call("mmvae_cluster_sil_sums", H.ptr(X), H.ptr(n2), H.ptr(column_list), H.ptr(table), H.ptr(first), H.ptr(ws), H.ptr(S),
           N, F, C, padded, n_chunks, H.stream())
    own = cnt[lab]
    a = S.gather(1, lab[:, None])[:, 0] / (own - 1).clamp(min=1)
    others = (cnt[None, :] > 0) & (torch.arange(C, device=dev)[None, :] != lab[:, None])
    b = torch.where(others, S / cnt.clamp(min=1)[None, :], torch.full_like(S, float("inf"))).min(1).values
    top = torch.maximum(a, b)
    s = torch.where((own > 1) & (top > 0), (b - a) / top, torch.zeros_like(top))
    return {"samples": s, "score": float(s.mean()), "sums": S, "counts": cnt}


def cluster_agreement(a, b):
    """Agreement of two labelings of the same rows, a the classes and b the clusters, from their integer contingency table
    T[class, cluster] on the host in float64, as scikit-learn defines them: adjusted Rand index, normalised mutual
    information (arithmetic mean of the entropies, natural logarithm), homogeneity, completeness, and purity = sum over
    the clusters of max_class T / N.  -> {"ari", "nmi", "homogeneity", "completeness", "purity"}: floats"""
    who = "cluster_agreement"
    sides = []
    for what, t in (("a", a), ("b", b)):
        sides.append(_cluster_labels(who, what, t, None)[0].cpu().numpy())
    if len(sides[0]) != len(sides[1]):
        raise ValueError(f"{who}: a has {len(sides[0])} entries, b {len(sides[1])} (one pair of ids per row)")
    ia, ib = (np.unique(t, return_inverse=True)[1] for t in sides)
    T = np.zeros((int(ia.max()) + 1, int(ib.max()) + 1), dtype=np.int64)
    np.add.at(T, (ia, ib), 1)
    N, ra, rb = int(T.sum()), T.sum(1), T.sum(0)
    sq = int((T * T).sum())
    tp, fp, fn = sq - N, int((T @ rb).sum()) - sq, int((T.T @ ra).sum()) - sq
    tn = N * N - fp - fn - sq
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    i, j = np.nonzero(T)
    v = T[i, j].astype(np.float64)
    mi = float(max(np.sum(v / N * (np.log(v) - math.log(N)) + v / N * (-np.log(ra[i] * rb[j].astype(np.float64))
                                                                       + 2.0 * math.log(N))), 0.0))

    def entropy(n):
        n = n[n > 0].astype(np.float64)
        return float(-np.sum((n / n.sum()) * (np.log(n) - math.log(n.sum()))))
    ha, hb, tiny = entropy(ra), entropy(rb), float(np.finfo(np.float64).eps)
    if len(ra) == 1 and len(rb) == 1:
        nmi = 1.0
    else:
        nmi = 0.0 if mi <= tiny else mi / max(0.5 * (ha + hb), tiny)
    return {"ari": float(ari), "nmi": float(nmi), "homogeneity": mi / ha if ha else 1.0,
            "completeness": mi / hb if hb else 1.0, "purity": float(T.max(0).sum()) / N}
