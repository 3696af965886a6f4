"""Extended-precision restatement of the aggregate posterior and of what is read from it: the ELBO
decomposition (index-code mutual information, total correlation, dimension-wise KL) and the mutual information gap of Chen
et al. 2018.  It shares nothing with the kernel: every pair term is computed in np.longdouble with a true division, every
log-sum-exp is taken against the MAXIMUM of its terms (the kernel shifts by the row's own term), the class sizes come from
a comparison of label vectors, and the walk goes in blocks of sample rows so that no temporary holds more than BLOCK_TERMS
terms.  Also the seeded case generator of the tests and the rounding bar.

The bar of every log-sum-exp output (joint, marginal, conditional), absolute, in nats: (16 * 745 + N) * 2^-53.  A sum of N
positive terms carries a relative error of at most its largest term error plus N u (u = 2^-53); a term that survives has an
argument of magnitude at most 745 (below -745 exp vanishes, in the kernel and here, whichever shift is taken), the argument
is a handful of double operations on numbers of that magnitude (difference, product with 1 / s, square or absolute value,
the constant, the shift: 16 u of it bounds them with room), and exp adds a few u; the logarithm turns the relative error of
the sum into absolute nats.  The kernel's joint adds D terms in sequence before its exp: each addition rounds a partial sum
whose magnitude stays within the same 745 for a surviving term, and the errors of the terms that carry the sum -- those
within some tens of nats of the largest -- are what the result sees, so that the same constant holds; the tests measure the
fraction that is used.
Scalars: mi, tc, dwkl are means of differences of (D + 2) such outputs at most: (D + 2) bars; entropies and the mutual
information table: 2 bars; mig_k = a difference of two table entries over H(v_k): 4 bars / H(v_k) (the gap between the
two largest is continuous in the table: a tie that swaps them changes nothing)."""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
BLOCK_TERMS = 2_000_000
HALF_LOG_2PI = LD(0.5) * np.log(LD(2) * LD(np.pi))

# (N, D, K, classes, laplace): below one row tile of 64, ragged against the row tile (64), the staged tile (32), the
# dimension block (16) and the chunks; D = 1; K = 0 (no labels) and K = the limit of 8; both families; more than one chunk
CASES = ((9, 1, 1, 2, False), (70, 5, 2, 3, True), (130, 16, 5, 4, False), (300, 33, 8, 3, True), (1100, 10, 3, 5, False),
         (70, 256, 2, 3, False), (257, 64, 0, 0, True))
IDS = [f"{n}x{d}k{k}{'L' if lap else 'N'}" for n, d, k, _, lap in CASES]


def bar(N):
    return (16 * 745 + N) * U


def generate(N, D, K, classes, laplace, seed=3, scale_lo=0.25, scale_hi=1.2):
    """-> (z, loc, scale (N,D) fp32, labels (K,N) int32 or None): loc = 0.4 noise + 1.5 (label_k - centre) on dimension k
    for k < min(K, D) + a weaker 0.7 carrier of factor 0 on dimension K when D > K; scale log-uniform in [scale_lo,
    scale_hi]; z = loc + scale e, e of the family; everything rounded to fp32"""
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, classes, size=(K, N)).astype(np.int32) if K > 0 else None
    loc = 0.4 * rng.standard_normal((N, D))
    if K > 0:
        centre = 0.5 * (classes - 1)
        for k in range(min(K, D)):
            loc[:, k] += 1.5 * (labels[k] - centre)
        if D > K:
            loc[:, K] += 0.7 * (labels[0] - centre)
    scale = np.exp(rng.uniform(np.log(scale_lo), np.log(scale_hi), size=(N, D)))
    e = rng.laplace(size=(N, D)) if laplace else rng.standard_normal((N, D))
    loc, scale = loc.astype(np.float32), scale.astype(np.float32)
    z = (loc.astype(np.float64) + scale.astype(np.float64) * e).astype(np.float32)
    return z, loc, scale, labels


def pair_terms(z, loc, scale, laplace):
    """l[n,m,d] (len(z), len(loc), D) in np.longdouble: log q(z_nd | x_m)"""
    z, loc, s = z.astype(LD)[:, None, :], loc.astype(LD)[None, :, :], scale.astype(LD)[None, :, :]
    t = (z - loc) / s
    if laplace:
        return -np.abs(t) - np.log(LD(2) * s)
    return -LD(0.5) * t * t - np.log(s) - HALF_LOG_2PI


def lse(l, axis):
    """log sum exp over `axis` against the maximum"""
    top = l.max(axis=axis, keepdims=True)
    return np.squeeze(top, axis) + np.log(np.exp(l - top).sum(axis=axis))


def aggregate(z, loc, scale, laplace, labels=None):
    """-> {"joint" (N,), "marginal" (N,D), "conditional" (K,N,D) | None, "self" (N,), "counts" (K,N)} in np.longdouble"""
    N, D = z.shape
    K = 0 if labels is None else len(labels)
    joint, marginal, own = np.empty(N, LD), np.empty((N, D), LD), np.empty(N, LD)
    cond = np.empty((K, N, D), LD) if K else None
    counts = np.empty((K, N), np.int64) if K else None
    log_n = np.log(LD(N))
    step = max(1, BLOCK_TERMS // (N * D))
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        l = pair_terms(z[lo:hi], loc, scale, laplace)
        joint[lo:hi] = lse(l.sum(2), 1) - log_n
        marginal[lo:hi] = lse(l, 1) - log_n
        own[lo:hi] = l[np.arange(hi - lo), np.arange(lo, hi)].sum(1)
        for k in range(K):
            for value in np.unique(labels[k][lo:hi]):      # the block's rows of one class against that class's columns
                rows, cols = np.nonzero(labels[k][lo:hi] == value)[0], np.nonzero(labels[k] == value)[0]
                counts[k, lo + rows] = len(cols)
                cond[k, lo + rows] = lse(l[rows][:, cols], 1) - np.log(LD(len(cols)))
    return {"joint": joint, "marginal": marginal, "conditional": cond, "self": own, "counts": counts}


def log_prior(z, loc=0.0, scale=1.0, laplace=False):
    """lpz (N,) in np.longdouble: sum_d log p(z_nd), p = Normal | Laplace (loc, scale) (scalars or (D,) arrays)"""
    prior_loc = np.broadcast_to(np.asarray(loc, LD), (1, z.shape[1]))
    prior_scale = np.broadcast_to(np.asarray(scale, LD), (1, z.shape[1]))
    l = pair_terms(z, prior_loc, prior_scale, laplace)
    return l[:, 0, :].sum(1)


def decomposition(agg, lpz):
    """{"mi", "tc", "dwkl", "kl"} in np.longdouble"""
    sum_marginal = agg["marginal"].sum(1)
    return {"mi": (agg["self"] - agg["joint"]).mean(), "tc": (agg["joint"] - sum_marginal).mean(),
            "dwkl": (sum_marginal - lpz).mean(), "kl": (agg["self"] - lpz).mean()}


def gap(agg, labels):
    """{"mig", "per_factor" (K,), "mi" (K,D), "h_z" (D,), "h_v" (K,)} in np.longdouble; D >= 2"""
    h_z = -agg["marginal"].mean(0)
    table = h_z[None, :] + agg["conditional"].mean(1)
    h_v = []
    for row in labels:
        p = np.bincount(row).astype(LD) / LD(len(row))
        p = p[p > 0]
        h_v.append(-(p * np.log(p)).sum())
    h_v = np.array(h_v, LD)
    top = np.sort(table, axis=1)
    per = (top[:, -1] - top[:, -2]) / h_v
    return {"mig": per.mean(), "per_factor": per, "mi": table, "h_z": h_z, "h_v": h_v}


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _solved(z, loc, scale, labels, laplace):
    z, loc, scale, labels = _frozen(z, loc, scale, labels)
    agg = aggregate(z, loc, scale, laplace, labels)
    out = {"z": z, "loc": loc, "scale": scale, "labels": labels, "laplace": laplace, "agg": agg,
           "lpz": log_prior(z)}
    out["elbo"] = decomposition(agg, out["lpz"])
    out["gap"] = gap(agg, labels) if labels is not None and z.shape[1] >= 2 else None
    return out


@functools.lru_cache(maxsize=None)
def case(i):
    """case i of CASES -> its inputs and everything restated from them (prior: the standard Normal), computed once and
    shared (treat as read-only)"""
    N, D, K, classes, laplace = CASES[i]
    return _solved(*generate(N, D, K, classes, laplace), laplace)


@functools.lru_cache(maxsize=None)
def special(name):
    """the edge cases, computed once and shared (read-only):
      underflow  scales log-uniform in [1e-3, 3]: most cross terms fall below -745 and vanish, exp arguments above the
                 row's own term reach +14 or so (what breaks an fp32 shift or a missing log s)
      single     sample 5 is the only member of its class of factor 0 (N_c = 1: its conditional is its own term)
      duplicate  rows 0 and 1 are one posterior and one draw"""
    if name == "underflow":
        return _solved(*generate(130, 16, 5, 4, False, scale_lo=1e-3, scale_hi=3.0), False)
    z, loc, scale, labels = generate(70, 5, 2, 3, name == "single")
    if name == "single":
        labels[0, 5] = 7
        return _solved(z, loc, scale, labels, True)
    assert name == "duplicate"
    z[1], loc[1], scale[1] = z[0], loc[0], scale[0]
    return _solved(z, loc, scale, labels, False)
