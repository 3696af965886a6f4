"""Extended-precision restatement of the kernel inception distance (Binkowski et al. 2018): the
unbiased MMD^2 between two feature sets under the polynomial kernel k(x, y) = (gamma x . y + c0)^p over random subsets.
Everything is numpy longdouble from the fp32 rows: the rows of a subset are gathered by fancy indexing (a copy -- what the
kernel never makes), the m x m blocks are written out, the power is `**`, the diagonal is taken out as a trace.  Also the
seeded inputs of the GPU tests (the feature generator of tests/manifold_reference.py, by import), the draw of the subsets,
the rounding bounds, and the condition on the inputs that makes those bounds a demand worth making."""
import functools

import numpy as np

from manifold_reference import sets

U = 2.0 ** -53
LD = np.longdouble
SEED = 5
# (N, M, F, m, S, shift, scale of the generated set), each the smallest at which one path of the kernel can go wrong:
# fewer rows than a tile and F no multiple of 4 | m = the whole smaller set, a ragged tile | two row tiles (off-diagonal
# tiles doubled), F = 4 staged steps + 2 | the longest F loop | five tiles: with chunks = 2, 3, 5 more than one chunk and
# more than one tile in a chunk | the same distribution twice (negative estimates)
SHAPES = ((9, 6, 5, 4, 3, 0.15, 0.9), (70, 45, 50, 45, 2, 0.15, 0.9), (130, 200, 130, 100, 3, 0.1, 0.95),
          (70, 45, 2048, 40, 2, 0.02, 1.0), (600, 500, 64, 300, 4, 0.15, 0.9), (600, 500, 64, 300, 4, 0.0, 1.0))
CHUNKED, SAME = 4, 5      # the shapes of the chunk plans and of the same-distribution case
# the hand-checkable integer case: F = 2, even coordinates, gamma = 1/2, c0 = 1, p = 3, m = 5: t = x . y / 2 + 1 is an
# integer, so is every kernel value and every sum (far below 2^53); the row (2, 0) occurs in both sets
INT_REAL = np.array([[0, 0], [2, 0], [0, 2], [2, 2], [4, 2], [2, 4]], dtype=np.float32)
INT_FAKE = np.array([[2, 0], [4, 4], [0, 4], [6, 2], [2, 6], [4, 0], [0, 6]], dtype=np.float32)
INT_IDX = (np.array([[0, 1, 2, 3, 4], [5, 3, 1, 4, 2]]), np.array([[0, 1, 2, 3, 4], [6, 5, 0, 2, 3]]))
INT_KERNEL = dict(degree=3, gamma=0.5, coef0=1.0)


def draw(n_real, n_fake, subsets, m, seed=SEED):
    """rs = RandomState(seed); for s in order: rs.choice(n_real, m, replace=False), then rs.choice(n_fake, m, replace=False)"""
    rs = np.random.RandomState(seed)
    idx_real, idx_fake = [], []
    for _ in range(subsets):
        idx_real.append(rs.choice(n_real, m, replace=False))
        idx_fake.append(rs.choice(n_fake, m, replace=False))
    return np.stack(idx_real), np.stack(idx_fake)


def gram(A, B, degree, gamma, coef0):
    """(len(A), len(B)) longdouble: (gamma a . b + coef0)^degree"""
    return (LD(gamma) * (A.astype(LD) @ B.astype(LD).T) + LD(coef0)) ** int(degree)


def sums(X, Y, idx_x, idx_y, degree=3, gamma=None, coef0=1.0):
    """(S, 3) longdouble: [sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i,j} k(x_i, y_j)] per subset, the
    diagonal left out by POSITION in the list (the trace of the gathered block)"""
    gamma = 1.0 / X.shape[1] if gamma is None else gamma
    out = np.empty((len(idx_x), 3), dtype=LD)
    for s, (ix, iy) in enumerate(zip(idx_x, idx_y)):
        Xs, Ys = X[ix], Y[iy]
        Kxx, Kyy, Kxy = (gram(A, B, degree, gamma, coef0) for A, B in ((Xs, Xs), (Ys, Ys), (Xs, Ys)))
        out[s] = Kxx.sum() - np.trace(Kxx), Kyy.sum() - np.trace(Kyy), Kxy.sum()
    return out


def mmd2(sm, m):
    sm = np.asarray(sm, dtype=LD)
    return sm[:, 0] / LD(m * (m - 1)) + sm[:, 1] / LD(m * (m - 1)) - 2 * sm[:, 2] / LD(m * m)


def kid(real, fake, subsets, subset_size, seed=SEED, idx=None, degree=3, gamma=None, coef0=1.0):
    """-> {"kid", "std" (divisor S), "mmd2" (S,), "sums" (S,3), "idx_real", "idx_fake", "m"}, longdouble"""
    m = min(subset_size, len(real), len(fake)) if idx is None else idx[0].shape[1]
    assert m >= 2
    idx_real, idx_fake = draw(len(real), len(fake), subsets, m, seed) if idx is None else idx
    sm = sums(real, fake, idx_real, idx_fake, degree, gamma, coef0)
    v = mmd2(sm, m)
    return {"kid": v.mean(), "std": np.sqrt(((v - v.mean()) ** 2).mean()), "mmd2": v, "sums": sm, "idx_real": idx_real,
            "idx_fake": idx_fake, "m": m}


# ---- rounding bounds (derived, not tuned) --------------------------------------------------------------------------------
# u = 2^-53, s2 = max |x|^2 over both sets, T = |gamma| s2 + |c0| >= |gamma x . y + c0| (Cauchy-Schwarz), n terms.
def bar_sum(F, m, degree, gamma, coef0, s2, n):
    """a sum of n kernel values in double: 2 (p (F + 3) + 2 m + 64) u n T^p.  An F-term dot bounded by s2 carries at most
    F u s2; t = gamma g + c0 two more roundings: relative to T at most (F + 2) u, which the p-th power multiplies by p, plus
    its own p - 1 roundings: p (F + 3) u T^p per term.  Every term then passes through at most 2 m + 64 additions (its row's
    partial over the columns, the partials of a slice: at most m each; the shuffles and the tree: far below 64), each
    rounding at most u times the running sum <= n T^p.  The factor 2 covers the second-order terms."""
    T = abs(gamma) * s2 + abs(coef0)
    return 2.0 * (degree * (F + 3) + 2 * m + 64) * U * n * T ** degree


def bar_mmd(F, m, degree, gamma, coef0, s2):
    """of one mmd2 = sxx / (m (m - 1)) + syy / (m (m - 1)) - 2 sxy / m^2: 4 bar_sum(n = m^2) / (m (m - 1)) -- sxx and syy
    once each, sxy twice, every sum of at most m^2 terms and every divisor at least m (m - 1); the three quotients and the
    two additions round far below that"""
    return 4.0 * bar_sum(F, m, degree, gamma, coef0, s2, m * m) / (m * (m - 1))


def bar_kid(b_mmd, mmd):
    """of the mean over the subsets: bar_mmd + 4 u max |mmd2| -- a mean moves by at most the largest change of a value;
    the device's own sum and division (pairwise summation in torch) round within 4 u of the largest magnitude"""
    return b_mmd + 4.0 * U * float(np.abs(mmd).max())


def bar_std(b_mmd):
    """the standard deviation (divisor S) is 1-Lipschitz in the largest change of a value; its own roundings are far below
    the second bar_mmd"""
    return 2.0 * b_mmd


def s2_of(X, Y):
    return float(max((X.astype(np.float64) ** 2).sum(1).max(), (Y.astype(np.float64) ** 2).sum(1).max()))


@functools.lru_cache(maxsize=None)
def case(i, degree=3, gamma=None, coef0=1.0):
    """shape i of SHAPES with the kernel (degree, gamma, coef0) -> (X, Y, idx_x, idx_y, ref, bars), computed once and
    shared (read-only).  ref = kid(...); bars = {"sum": per column (3,), "mmd", "kid", "std"}.  Asserts the condition on
    the inputs: every |mmd2[s]| >= 1e6 bar_mmd -- else choose other inputs."""
    N, M, F, m, S, shift, scale = SHAPES[i]
    X, Y = sets(N, M, F, shift, scale)
    ref = kid(X, Y, S, m, SEED, degree=degree, gamma=gamma, coef0=coef0)
    for a in (X, Y, ref["idx_real"], ref["idx_fake"], ref["mmd2"], ref["sums"]):
        a.setflags(write=False)
    g = 1.0 / F if gamma is None else gamma
    s2 = s2_of(X, Y)
    b_mmd = bar_mmd(F, m, degree, g, coef0, s2)
    bars = {"sum": np.array([bar_sum(F, m, degree, g, coef0, s2, n) for n in (m * (m - 1), m * (m - 1), m * m)]),
            "mmd": b_mmd, "kid": bar_kid(b_mmd, ref["mmd2"]), "std": bar_std(b_mmd)}
    ratio = float(np.abs(ref["mmd2"]).min()) / b_mmd
    assert ratio >= 1e6, f"shape {SHAPES[i]}: |mmd2| is {ratio:.3g} rounding bars: choose other inputs"
    return X, Y, ref["idx_real"], ref["idx_fake"], ref, bars
