"""Cross-modal retrieval of latents (csrc/retrieval.hip): float64 distances, exact ranks, forward only."""
import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["retrieval_pairs", "retrieval_ranks", "retrieval_summary", "retrieval_label_precision"]


def _retrieval_sets(who, what, X, like=None):
    """contiguous fp32 (S, N, D) or ValueError: shape, dtype, the limits, the shape and device of `like`, finite values"""
    sizes = (f"{what} is {{0}} sets of {{1}} x {{2}} (2 .. {H.RETRIEVAL_MAX_SETS} sets of 1 .. {H.RETRIEVAL_MAX_ROWS} rows of "
             f"1 .. {H.RETRIEVAL_MAX_DIM} dimensions are on the MI355X path)")
    return ck.rows(who, what, X, 3, "(S, N, D), one (N, D) set of rows per modality",
                   ((0, 2, H.RETRIEVAL_MAX_SETS, sizes), (1, 1, H.RETRIEVAL_MAX_ROWS, sizes), (2, 1, H.RETRIEVAL_MAX_DIM, sizes)),
                   None if like is None else ("loc", like))


def _retrieval_ints(who, what, t, form):
    """an integer tensor on the host from a tensor, an array or nested lists, or ValueError naming the `form` wanted"""
    if not torch.is_tensor(t):
        try:
            t = torch.from_numpy(np.ascontiguousarray(t))
        except TypeError:
            pass      # (no array of numbers: refused below by the name of its type)
    return ck.integers(who, what, t, None, form, to="host")


def retrieval_pairs(S):
    """every ordered pair (query set, gallery set) of S different sets, in lexicographic order: S (S - 1) pairs"""
    return [(a, b) for a in range(int(S)) for b in range(int(S)) if a != b]


def retrieval_ranks(loc, scale=None, pairs=None, match=None, metric="l2", keep=0, chunks=0):
    """Retrieval of one set of rows from another, for P ordered pairs of the S sets of `loc` (S, N, D) (the latent means of S
    modalities, say; `scale` (S, N, D) their standard deviations): per pair (query set, gallery set) and query row i, where
    does the gallery row match[i] -- the row of the same sample -- rank among all N gallery rows by distance to the query?
      metric "l2"      sum (mq - mg)^2                    "cosine"  1 - mq . mg / (|mq| |mg|), 1 when either norm is 0
             "w2"      sum (mq - mg)^2 + (sq - sg)^2      "skl"     KL(q || g) + KL(g || q) of diagonal Gaussians
      (w2, skl: `scale` is needed, > 0), in double from the fp32 values by direct differences; a pair's distance is a function
      of its two rows alone, so the comparisons are exact with respect to these distances.
    `pairs`: integer (P, 2) (query set, gallery set), the two different; None: retrieval_pairs(S).  `match`: integer (N,), -1
    for a row without a partner; None: the identity.  `keep` <= 16 nearest gallery rows are returned per query.
    -> {"d_match" (P, N) float64 (NaN without a partner), "less", "equal" (P, N) int32: the gallery rows other than the
        partner that are nearer / exactly as near (-1 without a partner), "nn_d" (P, N, keep) float64 ascending, "nn_idx" (P, N,
        keep) int32, ordered by (distance, index), padded with (+inf, -1) when N < keep, "pairs": the list of pairs}.
    The N x N distances are never written.  `chunks`: how many workgroups share a row's gallery rows (0: the default plan);
    the result does not depend on it, nor on what other pairs the call holds, bit for bit."""
    who = "retrieval_ranks"
    if metric not in H.RETRIEVAL_METRICS:
        raise ValueError(f"{who}: metric = {metric!r} ({', '.join(H.RETRIEVAL_METRICS)})")
    keep, chunks = int(keep), ck.chunks(who, chunks, "chunks of gallery rows")
    if not 0 <= keep <= H.RETRIEVAL_MAX_KEEP:
        raise ValueError(f"{who}: keep = {keep} neighbours (0 .. {H.RETRIEVAL_MAX_KEEP} are on the MI355X path)")
    loc = _retrieval_sets(who, "loc", loc)
    S, N, D = loc.shape
    if metric in ("w2", "skl"):
        if scale is None:
            raise ValueError(f"{who}: metric {metric!r} compares distributions and needs `scale`")
        scale = _retrieval_sets(who, "scale", scale, loc)
        if not bool((scale > 0).all()):
            raise ValueError(f"{who}: scale holds values that are not positive")
    else:
        scale = None      # (l2 and cosine read the means alone)
    if pairs is None:
        pairs = retrieval_pairs(S)
    pt = _retrieval_ints(who, "pairs", pairs, "an integer (P, 2) list of (query set, gallery set)")
    if pt.dim() != 2 or pt.shape[1] != 2 or not 1 <= pt.shape[0] <= H.RETRIEVAL_MAX_PAIRS:
        raise ValueError(f"{who}: pairs is {tuple(pt.shape)}; (P, 2) with 1 <= P <= {H.RETRIEVAL_MAX_PAIRS} pairs")
    if int(pt.min()) < 0 or int(pt.max()) >= S or bool((pt[:, 0] == pt[:, 1]).any()):
        raise ValueError(f"{who}: pairs must hold two different sets out of 0 .. {S - 1} per row")
    if match is not None:
        match = _retrieval_ints(who, "match", match, "an integer (N,) list of gallery rows, -1 for none")
        if tuple(match.shape) != (N,):
            raise ValueError(f"{who}: match is {tuple(match.shape)}; ({N},), one gallery row per query row")
        if int(match.min()) < -1 or int(match.max()) >= N:
            raise ValueError(f"{who}: match holds entries outside -1 .. {N - 1}")
    ck.need_gpu(who, "loc is", loc.device)
    dev, P = loc.device, pt.shape[0]
    pd = pt.to(device=dev, dtype=torch.int32).contiguous()
    md = None if match is None else match.to(device=dev, dtype=torch.int32).contiguous()
    ws = torch.empty(H.lib().mmvae_retrieval_ws_bytes(N, P, keep, chunks) // 8, dtype=torch.float64, device=dev)
    d_match = torch.empty(P, N, dtype=torch.float64, device=dev)
    less, equal = (torch.empty(P, N, dtype=torch.int32, device=dev) for _ in range(2))
    nn_d = torch.empty(P, N, keep, dtype=torch.float64, device=dev)
    nn_idx = torch.empty(P, N, keep, dtype=torch.int32, device=dev)
    H.call("mmvae_retrieval_ranks", H.ptr(loc), H.ptr(scale), H.ptr(pd), H.ptr(md), H.ptr(ws) if ws.numel() else None,
           H.ptr(d_match), H.ptr(less), H.ptr(equal), H.ptr(nn_d) if keep else None, H.ptr(nn_idx) if keep else None, N, D, S, P,
           H.RETRIEVAL_METRICS[metric], keep, chunks, H.stream())
    return {"d_match": d_match, "less": less, "equal": equal, "nn_d": nn_d, "nn_idx": nn_idx,
            "pairs": [tuple(r) for r in pt.tolist()]}


def _retrieval_ks(who, ks):
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1 or len(set(ks)) != len(ks):
        raise ValueError(f"{who}: ks = {ks} (different positive numbers of neighbours)")
    return ks


def retrieval_summary(less, equal, ks=(1, 5, 10), n_gallery=None):
    """Recall@k, median rank and their kin from the `less` and `equal` counts of retrieval_ranks; on the host.
    PESSIMISTIC ranks: rank = 1 + less + equal -- a gallery row exactly as near as the partner is counted as if it were nearer,
    so a tie never counts as a hit: N identical embeddings score rank N, not 1, and collapsed posteriors score at the far end
    rather than as perfect retrieval.  Rows without a partner (less < 0) are left out.  `n_gallery`: the gallery's rows
    (default: the number of query rows).  Per pair (one dict for (N,) counts, a list of P dicts for (P, N)):
      "recall@k" = share of rows with rank <= k, "chance@k" = min(k / n_gallery, 1), "median_rank", "mean_rank", "mrr" = mean
      1 / rank, "normalised_rank" = mean (rank - 1) / (n_gallery - 1) (0 best, 1 worst, 0.5 at chance; 0 for one gallery
      row), "tied_rows" = rows with equal > 0, "n" = rows with a partner (NaN everywhere but the chances when 0)."""
    who = "retrieval_summary"
    ks = _retrieval_ks(who, ks)
    less = _retrieval_ints(who, "less", less, "the integer (N,) or (P, N) counts of retrieval_ranks").numpy()
    equal = _retrieval_ints(who, "equal", equal, "the integer (N,) or (P, N) counts of retrieval_ranks").numpy()
    if less.shape != equal.shape or less.ndim not in (1, 2) or less.shape[-1] < 1:
        raise ValueError(f"{who}: less is {less.shape}, equal {equal.shape}; the (N,) or (P, N) counts of retrieval_ranks")
    if bool(((less < 0) != (equal < 0)).any()):
        raise ValueError(f"{who}: less and equal disagree on the rows without a partner")
    Ng = less.shape[-1] if n_gallery is None else int(n_gallery)
    most = int((less.astype(np.int64) + equal).max())
    if Ng < 1 or most >= Ng:
        raise ValueError(f"{who}: n_gallery = {Ng} rows for a row with less + equal = {most} other rows")

    def one(l, e):
        has = l >= 0
        rank = (1 + l[has].astype(np.int64) + e[has].astype(np.int64)).astype(np.float64)
        n = int(has.sum())
        out = {"n": n, "tied_rows": int((e[has] > 0).sum())}
        for k in ks:
            out[f"recall@{k}"] = float((rank <= k).mean()) if n else float("nan")
            out[f"chance@{k}"] = min(k / Ng, 1.0)
        out["median_rank"] = float(np.median(rank)) if n else float("nan")
        out["mean_rank"] = float(rank.mean()) if n else float("nan")
        out["mrr"] = float((1.0 / rank).mean()) if n else float("nan")
        out["normalised_rank"] = (float(((rank - 1.0) / (Ng - 1)).mean()) if Ng > 1 else 0.0) if n else float("nan")
        return out

    return one(less, equal) if less.ndim == 1 else [one(l, e) for l, e in zip(less, equal)]


def retrieval_label_precision(nn_idx, labels_q, labels_g, ks=(1, 5, 10)):
    """Do a query's nearest gallery rows carry its label?  nn_idx (N, keep): the neighbour lists of one pair from
    retrieval_ranks (-1: an empty slot); labels_q (N,), labels_g (gallery rows,) integers; every k of `ks` <= keep.  On the
    host -> {k: {"precision": the mean over the queries of the share of the (filled) first k slots that carry the query's
    label, "hit": the share of queries with at least one such row among them}}."""
    who = "retrieval_label_precision"
    ks = _retrieval_ks(who, ks)
    idx = _retrieval_ints(who, "nn_idx", nn_idx, "the integer (N, keep) neighbour lists of one pair").numpy()
    lq = _retrieval_ints(who, "labels_q", labels_q, "an integer (N,) list, one label per query row").numpy()
    lg = _retrieval_ints(who, "labels_g", labels_g, "an integer list, one label per gallery row").numpy()
    if idx.ndim != 2 or lq.shape != (idx.shape[0],) or lg.ndim != 1 or lg.shape[0] < 1:
        raise ValueError(f"{who}: nn_idx is {idx.shape}, labels_q {lq.shape}, labels_g {lg.shape}; (N, keep), (N,) and (gallery "
                         f"rows,)")
    if max(ks) > idx.shape[1]:
        raise ValueError(f"{who}: ks = {ks} for lists of keep = {idx.shape[1]} neighbours")
    if idx.size and (int(idx.min()) < -1 or int(idx.max()) >= lg.shape[0]):
        raise ValueError(f"{who}: nn_idx holds entries outside -1 .. {lg.shape[0] - 1}")
    filled = idx >= 0
    if not bool(filled[:, 0].all()):
        raise ValueError(f"{who}: a query has no neighbour at all")
    same = filled & (lg[np.where(filled, idx, 0)] == lq[:, None])
    out = {}
    for k in ks:
        share = same[:, :k].sum(1) / filled[:, :k].sum(1)
        out[k] = {"precision": float(share.mean()), "hit": float(same[:, :k].any(1).mean())}
    return out
