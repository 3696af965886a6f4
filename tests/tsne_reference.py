"""Exact t-SNE in numpy float64, written from the definitions in include/mmvae_hip.h (which are scikit-learn's
method="exact" path: _binary_search_perplexity, _joint_probabilities, _kl_divergence, _gradient_descent).  What the GPU
tests of csrc/tsne.hip are held to; test_tsne_host.py holds it to outputs recorded from scikit-learn itself
(tests/golden/tsne/).  `dtype=np.float32` runs the iteration in float32: what float32 alone costs."""
import numpy as np

EPS = 2.220446049250313e-16
EXAGGERATION, SWITCH_IT = 12.0, 250


def clustered(seed, N, D, C):
    """the fixtures' inputs: X = centres[i % C] + N(0,1), centres 3 N(0,1), float32"""
    rs = np.random.RandomState(seed)
    centres = 3.0 * rs.standard_normal((C, D))
    X = centres[np.arange(N) % C] + rs.standard_normal((N, D))
    return X.astype(np.float32), (np.arange(N) % C).astype(np.int64)


def default_init(N, seed=123):
    return (1e-4 * np.random.RandomState(seed).standard_normal((N, 2))).astype(np.float32)


def sqdist(X):
    """D2[i,j] = sum_d (x_id - x_jd)^2 in double, rounded to float32"""
    X = np.asarray(X, np.float32).astype(np.float64)
    out = np.zeros((X.shape[0], X.shape[0]))
    for d in range(X.shape[1]):
        t = X[:, None, d] - X[None, :, d]
        out += t * t
    return out.astype(np.float32)


def search_row(d_row, i, perplexity, trace=None):
    """the binary search of row i over its float32 squared distances -> (p_j / s, the beta the row was computed with, s,
    steps, took the s == 0 branch at beta = 1).  `trace` collects H - log(perplexity) of every step."""
    d = np.asarray(d_row, np.float32).astype(np.float64)
    keep = np.arange(d.shape[0]) != i
    want = np.log(perplexity)
    beta, lo, hi = 1.0, -np.inf, np.inf
    zero_first = False
    for step in range(100):
        p = np.where(keep, np.exp(-d * beta), 0.0)
        s = p.sum()
        if s == 0.0:
            s = 1e-8
            zero_first = zero_first or step == 0
        p = p / s
        diff = np.log(s) + beta * np.sum(d * p) - want
        used = beta
        if trace is not None:
            trace.append(diff)
        if abs(diff) <= 1e-5:
            break
        if diff > 0.0:
            lo = beta
            beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
        else:
            hi = beta
            beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
    return p, used, s, step + 1, zero_first


def conditional_p(D2, perplexity):
    """-> (C (N,N), beta (N,), steps (N,), per-row traces of H - log(perplexity), rows that met s == 0 at beta = 1)"""
    N = D2.shape[0]
    C, beta, steps, traces, zero = np.zeros((N, N)), np.zeros(N), np.zeros(N, np.int64), [], []
    for i in range(N):
        tr = []
        C[i], beta[i], _, steps[i], z = search_row(D2[i], i, perplexity, tr)
        traces.append(tr)
        if z:
            zero.append(i)
    return C, beta, steps, traces, zero


def joint_p(D2, perplexity):
    """-> (P (N,N) float64 before the rounding to float32, beta (N,))"""
    C, beta, *_ = conditional_p(D2, perplexity)
    P = C + C.T
    P = P / max(P.sum(), EPS)
    P = np.maximum(P, EPS)
    np.fill_diagonal(P, 0.0)
    return P, beta


def row_entropy_gap(d_row, i, beta, perplexity):
    """|H - log(perplexity)| of row i at precision beta"""
    d = np.asarray(d_row, np.float32).astype(np.float64)
    p = np.where(np.arange(d.shape[0]) != i, np.exp(-d * beta), 0.0)
    s = p.sum()
    s = 1e-8 if s == 0.0 else s
    return abs(np.log(s) + beta * np.sum(d * p / s) - np.log(perplexity))


def schedule(it, switch_it=SWITCH_IT):
    """(exaggeration, momentum) of iteration `it`"""
    return (EXAGGERATION, 0.5) if it < switch_it else (1.0, 0.8)


def forces(Y, P, ex, dtype=np.float64):
    """-> (g (N,2), KL, Z, min_{i != j} w_ij / Z) at the embedding Y with ex P"""
    Y, eP = np.asarray(Y).astype(dtype), (dtype(ex) * np.asarray(P).astype(dtype))
    off = ~np.eye(Y.shape[0], dtype=bool)
    diff = Y[:, None, :] - Y[None, :, :]
    w = np.where(off, dtype(1.0) / (dtype(1.0) + (diff * diff).sum(-1)), dtype(0.0))
    Z = w.sum(dtype=dtype)
    Q = np.maximum(w / Z, dtype(EPS))
    g = dtype(4.0) * (((eP - Q) * w)[:, :, None] * diff).sum(1, dtype=dtype)
    kl = np.sum(np.where(off, eP * np.log(np.maximum(eP, dtype(EPS)) / Q), dtype(0.0)), dtype=dtype)
    return g, kl, Z, (w[off] / Z).min()


def default_lr(N):
    return max(N / EXAGGERATION / 4.0, 50.0)


def step(state, P, it, lr, dtype=np.float64, switch_it=SWITCH_IT):
    """one iteration on state = (Y, upd, gains) -> (new state, g, KL, |g|, Z, the gain decisions, upd g)"""
    Y, upd, gains = (np.asarray(a).astype(dtype) for a in state)
    ex, mom = schedule(it, switch_it)
    g, kl, Z, _ = forces(Y, P, ex, dtype)
    prod = upd * g
    inc = prod < 0
    gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
    upd = dtype(mom) * upd - dtype(lr) * (gains * g)
    return (Y + upd, upd, gains), g, kl, np.sqrt(np.sum(g * g, dtype=dtype)), Z, inc, prod


def fresh(Y0, dtype=np.float64):
    Y0 = np.asarray(Y0).astype(dtype)
    return Y0, np.zeros_like(Y0), np.ones_like(Y0)


def run(state, P, it0, n_iter, lr, dtype=np.float64, record=(), switch_it=SWITCH_IT, track_w=False):
    """-> (state, log (n_iter,2) of (KL, |g|), {it: the state BEFORE iteration it} for it in record, the least w_ij / Z met if track_w)"""
    log, kept, wmin = np.zeros((n_iter, 2)), {}, np.inf
    for k in range(n_iter):
        it = it0 + k
        if it in record:
            kept[it] = tuple(a.copy() for a in state)
        state, _, kl, gn, _, _, _ = step(state, P, it, lr, dtype, switch_it)
        log[k] = kl, gn
        if track_w:
            wmin = min(wmin, forces(state[0], P, 1.0)[3])
    return state, log, kept, wmin


def embed(P, Y0, max_iter=1000, lr=None, n_iter_without_progress=300, min_grad_norm=1e-7, dtype=np.float64):
    """scikit-learn's two stages with its stopping rule -> (Y, KL at Y without exaggeration, iterations run, log)"""
    N = P.shape[0]
    lr = default_lr(N) if lr is None else lr
    state, logs, it, switch_it = fresh(Y0, dtype), [], 0, SWITCH_IT
    for stage_end, patience in ((SWITCH_IT, SWITCH_IT), (max_iter, n_iter_without_progress)):
        best, best_it = np.inf, it
        while it < stage_end:
            state, log, _, _ = run(state, P, it, 1, lr, dtype, switch_it=switch_it)
            logs.append(log)
            it += 1
            if it % 50 == 0:
                if log[0, 0] < best:
                    best, best_it = log[0, 0], it - 1
                elif it - 1 - best_it > patience:
                    break
                if log[0, 1] <= min_grad_norm:
                    break
        switch_it = min(switch_it, it)
    return state[0], forces(state[0], P, 1.0)[1], it, np.concatenate(logs)


def trustworthiness(X, Y, k=5):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors=k), Euclidean, restated"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    n = X.shape[0]
    dX = ((X[:, None] - X[None]) ** 2).sum(-1)
    dY = ((Y[:, None] - Y[None]) ** 2).sum(-1)
    np.fill_diagonal(dX, np.inf)
    np.fill_diagonal(dY, np.inf)
    order = np.argsort(dX, axis=1, kind="stable")
    rank = np.empty_like(order)
    rank[np.arange(n)[:, None], order] = np.arange(n)[None, :] + 1
    nn = np.argsort(dY, axis=1, kind="stable")[:, :k]
    t = np.maximum(rank[np.arange(n)[:, None], nn] - k, 0).sum()
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def neighbour_purity(Y, labels, k=5):
    """share of points whose k nearest neighbours in Y all carry the point's label"""
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None] - Y[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float(np.mean(np.all(labels[nn] == labels[:, None], axis=1)))
