"""Float64 numpy restatement of the Frechet-distance path (csrc/frechet.hip): what the GPU tests
are held to.  The seeded feature recipe of the fixtures, Chan's merge of batch moments, the round-robin one-sided Jacobi
with the kernels' rotation and stopping rule, and the distance by three routes: that Jacobi, numpy.linalg.eigh, and the
nuclear norm of the product of the centred, scaled feature matrices."""
import os

import numpy as np

EPS = 2.0 ** -52
TAU2 = 1e-30
MAX_SWEEPS = 30

# case -> (seed, F, N1, N2)
CASES = {"a": (101, 5, 7, 6), "b": (102, 64, 300, 200), "c": (103, 64, 40, 33), "d": (104, 130, 257, 190),
         "e": (105, 64, 300, 300), "f": (106, 512, 2000, 1500)}
SMALL = ("a", "b", "c", "d", "e")      # their features are stored in the fixtures; f's are regenerated from the seed
CONSTANT_COLUMN, DUPLICATED = 3, (6, 7)      # case d: column 3 is constant, column 7 repeats column 6


def features(name):
    """-> (X1 (N1,F), X2 (N2,F)) float32: relu(Z W + shift), so that covariances are correlated and non-negative as real
    activations are; the second set has wider latents and another shift."""
    seed, F, N1, N2 = CASES[name]
    rng = np.random.RandomState(seed)
    W = rng.standard_normal((F, F)) / np.sqrt(F)
    shift = 0.5 * rng.standard_normal(F)
    Z1 = rng.standard_normal((N1, F))
    Z2 = 0.3 + 1.2 * rng.standard_normal((N2, F))
    X1 = np.maximum(Z1 @ W + shift, 0.0).astype(np.float32)
    X2 = np.maximum(Z2 @ W + shift + 0.1, 0.0).astype(np.float32)
    if name == "d":
        for X in (X1, X2):
            X[:, CONSTANT_COLUMN] = 0.5
            X[:, DUPLICATED[1]] = X[:, DUPLICATED[0]]
    if name == "e":
        X2 = X1.copy()
    return X1, X2


def moments(X):
    """np.mean / np.cov of the float64-cast rows, as the reference's calculate_activation_statistics"""
    X = np.asarray(X, np.float64)
    return X.mean(0), np.atleast_2d(np.cov(X, rowvar=False))


def chan_state(F):
    return [0.0, np.zeros(F), np.zeros((F, F))]


def chan_update(state, X):
    """fold a batch into (n, mean, M2): the batch mean, the centred scatter, Chan's merge"""
    X = np.asarray(X, np.float64)
    n, mean, M2 = state
    nb = X.shape[0]
    mb = X.sum(0) / nb
    C = X - mb
    delta = mb - mean
    state[2] = M2 + (C.T @ C + np.outer(delta, delta) * (n * nb / (n + nb)))
    state[1] = mean + delta * (nb / (n + nb))
    state[0] = n + nb
    return state


def chan_finish(state):
    n, mean, M2 = state
    return mean.copy(), M2 / (n - 1.0)


def pairs(n, step):
    """the n / 2 disjoint pairs (p < q) of one step of the round-robin ordering over n (even) columns"""
    k = np.arange(1, n // 2)
    p = np.concatenate([[n - 1], (step + k) % (n - 1)])
    q = np.concatenate([[step], (step - k + (n - 1)) % (n - 1)])
    return np.minimum(p, q), np.maximum(p, q)


def jacobi(S, vectors=True, max_sweeps=MAX_SWEEPS):
    """One-sided Jacobi of the symmetric S with the kernels' rule -> (values = |A_j|, V or None, sweeps, counted rotations
    per sweep).  Rows of the working arrays are the columns the sweeps rotate.  RuntimeError at the cap."""
    S = np.asarray(S, np.float64)
    F = S.shape[0]
    A = S.copy()
    V = np.eye(F) if vectors else None
    n = F + (F & 1)
    floor2 = (F * EPS) ** 2 * (A * A).sum(1).max()
    counts = []
    for _ in range(max_sweeps):
        counted = 0
        for step in range(n - 1):
            p, q = pairs(n, step)
            keep = q < F
            p, q = p[keep], q[keep]
            P, Q = A[p], A[q]
            a, b, c = (P * P).sum(1), (Q * Q).sum(1), (P * Q).sum(1)
            rot = (c != 0.0) & (c * c > TAU2 * a * b)
            if not rot.any():
                continue
            p, q, P, Q, a, b, c = p[rot], q[rot], P[rot], Q[rot], a[rot], b[rot], c[rot]
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                zeta = (b - a) / (2.0 * c)
                t = 1.0 / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            t = np.where(np.isnan(t), 0.0, t)
            t = np.where(zeta < 0.0, -t, t)
            cs = 1.0 / np.sqrt(1.0 + t * t)
            sn = cs * t
            A[p], A[q] = cs[:, None] * P - sn[:, None] * Q, sn[:, None] * P + cs[:, None] * Q
            if vectors:
                U, W = V[p], V[q]
                V[p], V[q] = cs[:, None] * U - sn[:, None] * W, sn[:, None] * U + cs[:, None] * W
            counted += int(((a > floor2) & (b > floor2)).sum())
        counts.append(counted)
        if counted == 0:
            break
    else:
        raise RuntimeError(f"jacobi: no convergence within {max_sweeps} sweeps (counted rotations {counts})")
    return np.sqrt((A * A).sum(1)), (V.T.copy() if vectors else None), len(counts), counts


def _assemble(mu1, s1, mu2, s2, tr_covmean):
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * tr_covmean)


def distance_jacobi(mu1, s1, mu2, s2):
    """the kernels' route -> (d^2, tr covmean, (sweeps of sigma1, sweeps of G))"""
    lam, V, sw1, _ = jacobi(s1)
    R = np.sqrt(lam)[:, None] * V.T
    G = R @ (s2 @ R.T)
    sv, _, sw2, _ = jacobi(G, vectors=False)
    tr = float(np.sqrt(sv).sum())
    return _assemble(mu1, s1, mu2, s2, tr), tr, (sw1, sw2)


def distance_eigh(mu1, s1, mu2, s2):
    """the same route on numpy.linalg.eigh (negative rounding noise clipped at 0) -> (d^2, tr covmean)"""
    lam, V = np.linalg.eigh(s1)
    R = np.sqrt(np.maximum(lam, 0.0))[:, None] * V.T
    G = R @ s2 @ R.T
    tr = float(np.sqrt(np.maximum(np.linalg.eigvalsh(0.5 * (G + G.T)), 0.0)).sum())
    return _assemble(mu1, s1, mu2, s2, tr), tr


def distance_nuclear(X1, X2):
    """a third, independent route: with A = (X1 - mean) / sqrt(N1 - 1) and B likewise, S1 = A^T A, S2 = B^T B and
    tr (S1 S2)^1/2 = the nuclear norm of A B^T (no covariance is squared or rooted) -> (d^2, tr covmean)"""
    X1, X2 = np.asarray(X1, np.float64), np.asarray(X2, np.float64)
    mu1, mu2 = X1.mean(0), X2.mean(0)
    A = (X1 - mu1) / np.sqrt(X1.shape[0] - 1.0)
    B = (X2 - mu2) / np.sqrt(X2.shape[0] - 1.0)
    tr = float(np.linalg.svd(A @ B.T, compute_uv=False).sum())
    d = mu1 - mu2
    return float(d @ d + (A * A).sum() + (B * B).sum() - 2.0 * tr), tr


def rel(x, y, scale=None):
    """relative deviation of two distances (of `scale` where the distance itself cancels to nothing, case e)"""
    return abs(x - y) / (max(abs(x), abs(y)) if scale is None else scale)


# ---- the fixtures of tests/golden/frechet and what the tests of a case share ---------------------------------------------------
BAR_FLOOR = 1e-12      # a case's bar: 4 x the spread of the independent routes, not below this
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frechet")
_MEMO = {}


def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def case(name):
    """everything the tests of a case share, computed once: features, float64 moments, the recorded value, the three
    routes of the restatement and the case's bar"""
    if name in _MEMO:
        return _MEMO[name]
    fx = fixture(name)
    X1, X2 = features(name)
    (mu1, s1), (mu2, s2) = moments(X1), moments(X2)
    # case e: d^2 cancels to rounding noise, deviations are taken relative to what cancels
    scale = float(np.trace(s1) + np.trace(s2)) if name == "e" else None
    rec = float(fx["distance"])
    eigh, _ = distance_eigh(mu1, s1, mu2, s2)
    nuc, _ = distance_nuclear(X1, X2)
    if name in SMALL:
        jac, tr_jac, sweeps = distance_jacobi(mu1, s1, mu2, s2)
    else:      # case f: 2 x 511 steps a sweep in numpy take half a minute: READ as the golden script recorded them from
               # distance_jacobi, not recomputed here (the eigh and nuclear-norm routes above are)
        jac, tr_jac = float(fx["restated_distance"]), float(fx["restated_tr_covmean"])
        sweeps = tuple(int(s) for s in fx["restated_sweeps"])
    spread = max(rel(rec, eigh, scale), rel(rec, nuc, scale), rel(eigh, nuc, scale))
    out = {"fx": fx, "X1": X1, "X2": X2, "mu1": mu1, "s1": s1, "mu2": mu2, "s2": s2, "scale": scale, "recorded": rec,
           "eigh": eigh, "nuclear": nuc, "jacobi": jac, "tr_jacobi": tr_jac, "sweeps": sweeps, "spread": spread,
           "bar": max(4.0 * spread, BAR_FLOOR)}
    _MEMO[name] = out
    return out
