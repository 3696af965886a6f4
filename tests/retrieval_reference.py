"""A float64 numpy restatement of the cross-modal retrieval of latents (csrc/retrieval.hip): the four
distances by direct differences with the dimensions summed in order, the ranks with their ties, the neighbour lists ordered
by (distance, index), and the summary.  Shared by tests/test_retrieval_host.py and tests/test_retrieval_gpu.py; nothing here
reads the code under test.

The rounding bar.  With u = 2^-53, a distance is a sum of D terms, each a handful of correctly rounded operations on
exactly converted fp32 values: l2 and w2 terms carry at most 3 u of relative error, an skl term (two squares, a reciprocal,
two products, the half) at most 8 u, and a sum of D terms taken in order adds (D - 1) u of the sum of the terms'
magnitudes.  So a distance computed in float64 in ANY order of roundings lies within (D + 8) u A of the exact value, where
A = the sum of the magnitudes of the terms:
  l2, w2   A = the distance itself (every term is >= 0)
  skl      A = sum_d 1/2 [..] + D       (the D ones that are taken off count as terms)
  cosine   A = 1 + 2 sum_d |mq mg| / (|mq| |mg|)  (the dot product (D + 1) u sum |mq mg|, each squared norm (D + 1) u
           relative, their product, the root and the quotient 3 u more, the final difference u: together below
           (D + 8) u A)
Both the kernel and this restatement are such computations, so they differ by at most bar = 2 (D + 8) u A.  `fair` then
asserts, from the restatement alone, what makes an EXACT comparison of ranks and neighbour indices legitimate -- every
decision the kernel takes has a margin of 10^3 bars -- and that the case tells something."""
import functools

import numpy as np

U = 2.0 ** -53
METRICS = ("l2", "cosine", "w2", "skl")
MARGIN = 1e3      # bars between two distances whose order is compared exactly

# (N, D): rows and columns at and around the tile edges (64 query rows, 32 staged gallery rows, 8 per wave), width 1, widths
# that are no multiple of the staged depth (32; skl: 16), and the largest width
SHAPES = ((1, 1), (63, 1), (64, 8), (65, 33), (130, 256), (200, 32))


def pair_distances(metric, ql, qs, gl, gs):
    """query rows (Nq, D) against gallery rows (Ng, D), fp32 means (and scales, or None) -> (d, bar) float64 (Nq, Ng)"""
    ql, gl = np.asarray(ql, np.float64), np.asarray(gl, np.float64)
    (Nq, D), Ng = ql.shape, gl.shape[0]
    if metric in ("w2", "skl"):
        qs, gs = np.asarray(qs, np.float64), np.asarray(gs, np.float64)
    acc, mag = np.zeros((Nq, Ng)), np.zeros((Nq, Ng))
    nq, ng = np.zeros((Nq, 1)), np.zeros((1, Ng))
    for d in range(D):
        a, b = ql[:, d:d + 1], gl[None, :, d]
        if metric == "cosine":
            acc, mag = acc + a * b, mag + np.abs(a * b)
            nq, ng = nq + a * a, ng + b * b
            continue
        diff = a - b
        if metric == "l2":
            term = diff * diff
        elif metric == "w2":
            e = qs[:, d:d + 1] - gs[None, :, d]
            term = diff * diff + e * e
        else:
            vq, vg = qs[:, d:d + 1] ** 2, gs[None, :, d] ** 2
            term = 0.5 * ((vq + diff * diff) / vg + (vg + diff * diff) / vq)
        acc, mag = acc + term, mag + term
    if metric == "cosine":
        den = np.sqrt(nq * ng)
        zero = (nq == 0) | (ng == 0)
        safe = np.where(zero, 1.0, den)
        acc, mag = np.where(zero, 1.0, 1.0 - acc / safe), np.where(zero, 1.0, 1.0 + 2.0 * mag / safe)
    elif metric == "skl":
        acc, mag = acc - D, mag + D
    return acc, 2.0 * (D + 8) * U * mag


def ranks(d, match=None):
    """-> (d_match (Nq,), less, equal (Nq,) int32): the columns other than the partner nearer / exactly as near; NaN and
    -1, -1 for match[i] == -1.  match None: the identity."""
    Nq, Ng = d.shape
    match = np.arange(Nq) if match is None else np.asarray(match)
    has = match >= 0
    m = np.where(has, match, 0)
    dm = d[np.arange(Nq), m]
    other = np.ones((Nq, Ng), bool)
    other[np.arange(Nq), m] = False
    less = ((d < dm[:, None]) & other).sum(1).astype(np.int32)
    equal = ((d == dm[:, None]) & other).sum(1).astype(np.int32)
    return np.where(has, dm, np.nan), np.where(has, less, -1).astype(np.int32), np.where(has, equal, -1).astype(np.int32)


def neighbours(d, keep):
    """-> (nn_d (Nq, keep) float64, nn_idx (Nq, keep) int32): the keep nearest columns by (distance, index), padded with
    (+inf, -1)"""
    Nq, Ng = d.shape
    nn_d, nn_idx = np.full((Nq, keep), np.inf), np.full((Nq, keep), -1, np.int32)
    for i in range(Nq):
        order = np.lexsort((np.arange(Ng), d[i]))[:keep]
        nn_d[i, :len(order)], nn_idx[i, :len(order)] = d[i, order], order
    return nn_d, nn_idx


def summary(less, equal, ks, n_gallery):
    """pessimistic ranks 1 + less + equal over the rows with a partner -> the fields of ops.retrieval_summary"""
    has = less >= 0
    rank = 1.0 + less[has].astype(np.float64) + equal[has]
    out = {"n": int(has.sum()), "tied_rows": int((equal[has] > 0).sum())}
    for k in ks:
        out[f"recall@{k}"], out[f"chance@{k}"] = float(np.mean(rank <= k)), min(k / n_gallery, 1.0)
    out.update(median_rank=float(np.median(rank)), mean_rank=float(rank.mean()), mrr=float(np.mean(1.0 / rank)),
               normalised_rank=float(np.mean((rank - 1.0) / (n_gallery - 1))) if n_gallery > 1 else 0.0)
    return out


def label_precision(nn_idx, labels_q, labels_g, ks):
    out = {}
    for k in ks:
        share, hit = [], []
        for i in range(nn_idx.shape[0]):
            rows = [j for j in nn_idx[i, :k] if j >= 0]
            same = [labels_g[j] == labels_q[i] for j in rows]
            share.append(sum(same) / len(rows))
            hit.append(any(same))
        out[k] = {"precision": float(np.mean(share)), "hit": float(np.mean(hit))}
    return out


def noise_of(D):
    """the standard deviation of the query noise: large enough that a query's partner is NOT its nearest row most of the
    time (with 0.3 nearly every rank is 1 from D = 8 up, and a kernel that returns zeros would pass).  For l2, a stranger's
    squared distance exceeds the partner's by |g_m - g_j|^2 + 2 noise n . (g_m - g_j): mean 2 D, deviation 2 noise sqrt(2 D);
    noise = sqrt(2 D) / 2.5 puts the mean at 1.25 deviations, so that a fair share of the strangers come nearer."""
    return max(1.5, float(np.sqrt(2.0 * D)) / 2.5)


@functools.lru_cache(maxsize=None)
def case(N, D, S=2, seed=0):
    """random fp32 sets: set 0 is the gallery, loc ~ N(0, 1), scale in [0.1, 1]; every other set is that set permuted plus
    noise (scales: permuted, times a factor in [1/2, 2], back into [0.1, 1]); match = the permutation of set 1 (query row i's
    partner is gallery row match[i] when set 1 queries set 0).  Read-only arrays."""
    rs = np.random.RandomState(1000 * N + 10 * D + seed)
    loc, scale = np.empty((S, N, D), np.float32), np.empty((S, N, D), np.float32)
    loc[0] = rs.standard_normal((N, D))
    scale[0] = rs.uniform(0.1, 1.0, (N, D))
    match = rs.permutation(N).astype(np.int32)
    for s in range(1, S):
        loc[s] = loc[0][match] + noise_of(D) * rs.standard_normal((N, D))
        scale[s] = np.clip(scale[0][match] * np.exp2(rs.uniform(-1.0, 1.0, (N, D))), 0.1, 1.0)
    for a in (loc, scale, match):
        a.setflags(write=False)
    return {"loc": loc, "scale": scale, "match": match, "N": N, "D": D, "S": S}


@functools.lru_cache(maxsize=None)
def reference(N, D, metric, q=1, g=0, S=2, seed=0, keep=16):
    """the restatement of set q querying set g of case(N, D, S, seed), partners by the case's permutation (for q = 1, g = 0;
    callers with other pairs pass their own match to `ranks`) -> dict of read-only arrays"""
    c = case(N, D, S, seed)
    d, bar = pair_distances(metric, c["loc"][q], c["scale"][q], c["loc"][g], c["scale"][g])
    dm, less, equal = ranks(d, c["match"])
    nn_d, nn_idx = neighbours(d, keep)
    out = {"d": d, "bar": bar, "d_match": dm, "less": less, "equal": equal, "nn_d": nn_d, "nn_idx": nn_idx}
    for a in out.values():
        a.setflags(write=False)
    return out


def fair(d, bar, match, keep, what=""):
    """The preconditions of an exact comparison, from the restatement alone:
      1. every row's matched distance is >= MARGIN bars (the larger of the two) away from every other distance of its row;
      2. the gaps among each row's keep + 1 smallest distances are >= MARGIN bars;
      3. the case is not trivial (N >= 4; one to three rows cannot be): the ranks take at least min(8, N / 4) distinct values
         and fewer than half the rows have rank 1.
    -> the smallest margin met, in bars."""
    Nq, Ng = d.shape
    match = np.arange(Nq) if match is None else np.asarray(match)
    worst = np.inf
    for i in range(Nq):
        m = match[i]
        if m >= 0 and Ng > 1:
            gap = np.abs(d[i] - d[i, m]) / np.maximum(bar[i], bar[i, m])
            gap[m] = np.inf
            worst = min(worst, float(gap.min()))
        order = np.lexsort((np.arange(Ng), d[i]))[:keep + 1]
        if len(order) > 1:
            dd, bb = d[i, order], bar[i, order]
            worst = min(worst, float(((dd[1:] - dd[:-1]) / np.maximum(bb[1:], bb[:-1])).min()))
    assert worst >= MARGIN, f"{what}: two distances {worst:.3g} bars apart: choose other inputs"
    _, less, equal = ranks(d, match)
    rank = 1 + less[less >= 0] + equal[less >= 0]
    if Nq >= 4:
        distinct, first = len(np.unique(rank)), int((rank == 1).sum())
        assert distinct >= min(8, Nq / 4) and 2 * first < len(rank), \
            f"{what}: {distinct} distinct ranks, {first} of {len(rank)} rows at rank 1: the case tells nothing"
    return worst


# ---- ties that are exact in both arithmetics: small-integer means, power-of-two scales ----------------------------------------------
def tie_case(N=70, D=6, dup=5, seed=3):
    """gallery rows of small integers with power-of-two scales; the rows dup .. 2 dup - 1 repeat the rows 0 .. dup - 1, the last
    row repeats row 0 too; the queries are the gallery rows themselves moved by small integers.  Every product, square,
    reciprocal and sum of these values is exact in double, whatever the order."""
    rs = np.random.RandomState(seed)
    loc = rs.randint(-4, 5, (2, N, D)).astype(np.float32)
    scale = np.exp2(rs.randint(-2, 2, (2, N, D))).astype(np.float32)
    loc[0, dup:2 * dup], scale[0, dup:2 * dup] = loc[0, :dup], scale[0, :dup]
    loc[0, N - 1], scale[0, N - 1] = loc[0, 0], scale[0, 0]
    loc[1], scale[1] = loc[0] + rs.randint(-1, 2, (N, D)), scale[0]
    loc[1, :2 * dup], loc[1, N - 1] = loc[0, :2 * dup], loc[0, N - 1]      # (these queries sit ON their duplicated rows)
    return {"loc": loc, "scale": scale, "N": N, "D": D, "dup": dup}
