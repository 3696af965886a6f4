"""Float64 numpy / scipy restatement of the cross-modal correlation, written from the formulae: the
yardstick of tests/test_cca_host.py and tests/test_cca_gpu.py.  Nothing here calls the library.

Two independent routes to the fit:
  (i)  route_eig       A and B assembled as the reference's cca does (B: the views' covariances on the block diagonal, A:
                       the off-diagonal blocks, `ridge` on both diagonals), then scipy.linalg.eig(A, B), the call it makes;
  (ii) route_whitened  per view B_i = Q L Q^T (numpy.linalg.eigh), W = blockdiag(Q L^-1/2 Q^T), N = W (sigma + 2 ridge I) W,
                       numpy.linalg.eigh(N): eigenvalues 1 + lambda, v = W u scaled to unit norm.
Also the cosine score, the frequency-weighted sentence feature and the fixed-order sum, in float64."""
import functools

import numpy as np
import scipy.linalg

EPS = 2.0 ** -52
U = 2.0 ** -53
CLAMP = 1e-8

# name: (widths, rows of the fit, k, seed); latent-factor data, full rank, rows >= 4 O
CASES = {"odd": ((7, 5), 200, 4, 11),            # odd widths: the solver's padding column
         "edge": ((130, 17), 600, 16, 12),       # across the 64 and 128 tile edges; 17 is no multiple of the MFMA k-step
         "three": ((9, 6, 5), 150, 5, 13),       # three views: values up to V - 1
         "stream": ((20, 12), 300, 6, 14)}       # folded as 128 + 128 + 44 rows and as one batch
SCORE_ROWS = 200
RIDGE = 1e-12


def latent_views(widths, rows, seed, deficient=False):
    """views (rows, o_i) float32 sharing d = min(widths) latent factors of graded strength (so that the canonical
    correlations are spread out) under unit noise; `deficient`: the last column of every view repeats its first"""
    rng = np.random.RandomState(seed)
    d = min(widths)
    z = rng.standard_normal((rows, d)) * np.geomspace(3.0, 0.3, d)
    mix = [rng.standard_normal((d, o)) / np.sqrt(d) for o in widths]
    shift = [rng.standard_normal(o) for o in widths]
    return mix, shift, _draw(rng, z, mix, shift, deficient)


def _draw(rng, z, mix, shift, deficient=False):
    views = [(z @ m + rng.standard_normal((len(z), m.shape[1])) + s).astype(np.float32) for m, s in zip(mix, shift)]
    if deficient:
        for v in views:
            v[:, -1] = v[:, 0]
    return views


def moments(views):
    """(mu, sigma) float64 of the rows that hold the float32 views side by side (np.cov's normalisation)"""
    X = np.concatenate([v.astype(np.float64) for v in views], axis=1)
    mu = X.mean(axis=0)
    Xc = X - mu
    return mu, Xc.T @ Xc / (len(X) - 1)


def _blocks(widths):
    offs = np.concatenate([[0], np.cumsum(widths)])
    return list(zip(offs[:-1], offs[1:]))


def assemble(sigma, widths, ridge):
    A, B = sigma.copy(), np.zeros_like(sigma)
    for lo, hi in _blocks(widths):
        B[lo:hi, lo:hi] = sigma[lo:hi, lo:hi]
        A[lo:hi, lo:hi] = 0.0
    A[np.diag_indices_from(A)] += ridge
    B[np.diag_indices_from(B)] += ridge
    return A, B


def route_eig(sigma, widths, k, ridge=RIDGE):
    """-> (correlations (k,), stacked projections (O, k) with unit columns, every value sorted descending)"""
    A, B = assemble(sigma, widths, ridge)
    values, vectors = scipy.linalg.eig(A, B)
    assert np.abs(values.imag).max() <= 1e-9 * np.abs(values.real).max()
    order = np.argsort(values.real)[::-1]
    P = vectors.real[:, order[:k]]
    return values.real[order[:k]], P / np.linalg.norm(P, axis=0), values.real[order]


def route_whitened(sigma, widths, k, ridge=RIDGE):
    O = sigma.shape[0]
    W = np.zeros_like(sigma)
    for lo, hi in _blocks(widths):
        lam, Q = np.linalg.eigh(sigma[lo:hi, lo:hi] + ridge * np.eye(hi - lo))
        W[lo:hi, lo:hi] = (Q / np.sqrt(lam)) @ Q.T
    N = W @ (sigma + 2.0 * ridge * np.eye(O)) @ W
    values, vectors = np.linalg.eigh((N + N.T) / 2)
    order = np.argsort(values)[::-1]
    P = W @ vectors[:, order[:k]]
    return values[order[:k]] - 1.0, P / np.linalg.norm(P, axis=0), values[order] - 1.0


def kappa(sigma, widths, ridge=RIDGE):
    """max_i lambda_max(B_i) / lambda_min(B_i), and the per-view lambda_min / lambda_max"""
    lam = [np.linalg.eigvalsh(sigma[lo:hi, lo:hi] + ridge * np.eye(hi - lo)) for lo, hi in _blocks(widths)]
    return max(l[-1] / l[0] for l in lam), [l[0] / l[-1] for l in lam]


def min_gap(all_values, k):
    """the smallest gap between adjacent kept values, the gap of the k-th to the first one left out included (a column
    is only defined as far as its value is apart from BOTH neighbours)"""
    return float(np.min(-np.diff(all_values[:k + 1])))


def align_signs(P, ref):
    """P with each column's sign chosen to agree with `ref`"""
    s = np.sign(np.sum(P * ref, axis=0))
    return P * np.where(s == 0, 1.0, s)


def split(P, widths):
    return [P[lo:hi] for lo, hi in _blocks(widths)]


def cosine_scores(a, b, mean_a, mean_b, Pa, Pb):
    """per row cos = p . q / (max(|p|, 1e-8) max(|q|, 1e-8)); also the clamped norm products"""
    p = (a.astype(np.float64) - mean_a) @ Pa
    q = (b.astype(np.float64) - mean_b) @ Pb
    prod = np.maximum(np.linalg.norm(p, axis=1), CLAMP) * np.maximum(np.linalg.norm(q, axis=1), CLAMP)
    return np.sum(p * q, axis=1) / prod, prod


def fixed_order_sum(cos):
    """thread t of 256 adds the rows t, t + 256, ... in order; the partials are added in thread order"""
    total = 0.0
    for t in range(256):
        s = 0.0
        for v in cos[t::256]:
            s += float(v)
        total = s if t == 0 else total + s
    return total


def sentence_features(ids, emb, weights, eos=2, pc=None):
    """(B, E) float64: the weighted mean of the embeddings up to and including the first eos, minus its part along pc"""
    out = np.zeros((len(ids), emb.shape[1]))
    for r, s in enumerate(np.asarray(ids)):
        hit = np.where(s == eos)[0]
        L = hit[0] + 1 if len(hit) else len(s)
        f = np.zeros(emb.shape[1])
        for t in s[:L]:
            f += float(weights[t]) * emb[t].astype(np.float64)
        f /= L
        out[r] = f if pc is None else f - pc * (pc @ f)
    return out


def top_component(feats):
    """top right singular vector of the centred float64 features, and the relative gap (l1 - l2) / l1 of the covariance's
    two largest eigenvalues"""
    X = feats.astype(np.float64)
    _, s, Vt = np.linalg.svd(X - X.mean(axis=0), full_matrices=False)
    l1, l2 = s[0] ** 2, (s[1] ** 2 if len(s) > 1 else 0.0)
    return Vt[0], (l1 - l2) / l1


@functools.lru_cache(maxsize=None)
def case(name, ridge=RIDGE, deficient=False):
    """everything the tests need of a case, computed once: the fit's views and moments, both routes, the bars, SCORE_ROWS
    further pairs from the same generator and their scores under both routes"""
    widths, rows, k, seed = CASES[name]
    mix, shift, views = latent_views(widths, rows, seed, deficient)
    mu, sigma = moments(views)
    v1, P1, all1 = route_eig(sigma, widths, k, ridge)
    v2, P2, all2 = route_whitened(sigma, widths, k, ridge)
    P2 = align_signs(P2, P1)
    O = sum(widths)
    kap, condition = kappa(sigma, widths, ridge)
    gap = min_gap(all1, k)
    rng = np.random.RandomState(seed + 1000)
    d = min(widths)
    test = _draw(rng, rng.standard_normal((SCORE_ROWS, d)) * np.geomspace(3.0, 0.3, d), mix, shift, deficient)
    means = split(mu, widths)
    s1, prod = cosine_scores(test[0], test[1], means[0], means[1], split(P1, widths)[0], split(P1, widths)[1])
    s2, _ = cosine_scores(test[0], test[1], means[0], means[1], split(P2, widths)[0], split(P2, widths)[1])
    bar_values = 4 * O * EPS * kap
    return {"widths": widths, "rows": rows, "k": k, "O": O, "views": views, "mu": mu, "sigma": sigma, "means": means,
            "values": v1, "P": P1, "values_whitened": v2, "P_whitened": P2, "kappa": kap, "condition": condition,
            "gap": gap, "bar_values": bar_values, "bar_projections": bar_values / gap, "test": test,
            "scores": s1, "scores_whitened": s2, "norm_products": prod,
            "spread_values": float(np.abs(v1 - v2).max()), "spread_projections": float(np.abs(P1 - P2).max()),
            "spread_rows": float(np.abs(s1 - s2).max()), "spread_mean": float(abs(s1.mean() - s2.mean()))}


def score_bar(spread_rows, oa, ob, k, norm_products):
    """per-row bar of the score kernel: the larger of 8 x the spread of the two float64 routes and the rounding bound
    4 (o_a + o_b + k) 2^-53 over the smallest clamped norm product of the case"""
    return max(8.0 * spread_rows, 4 * (oa + ob + k) * U / float(np.min(norm_products)))


def mean_score_bar(c, fa, fb):
    """bar of a row's score (and so of a mean of rows) under the DEVICE's fit against the restatement's: the score kernel's
    own bar plus what moving every element of the projections by bar_projections can do to a cosine.  With p = x P,
    |dp| <= |x| sqrt(o k) bar, and the cosine of two vectors moves by at most |dp| / |p| + |dq| / |q| to first order
    (margin 2); the largest over the rows.  c: a case (its first two views)."""
    (oa, ob), k = c["widths"][:2], c["k"]
    Pa, Pb = split(c["P"], c["widths"])[:2]
    xa, xb = fa.astype(np.float64) - c["means"][0], fb.astype(np.float64) - c["means"][1]
    _, prod = cosine_scores(fa, fb, c["means"][0], c["means"][1], Pa, Pb)
    np_, nq = np.maximum(np.linalg.norm(xa @ Pa, axis=1), CLAMP), np.maximum(np.linalg.norm(xb @ Pb, axis=1), CLAMP)
    moved = 2.0 * c["bar_projections"] * (np.linalg.norm(xa, axis=1) * np.sqrt(oa * k) / np_
                                          + np.linalg.norm(xb, axis=1) * np.sqrt(ob * k) / nq)
    return score_bar(c["spread_rows"], oa, ob, k, prod) + float(moved.max())
