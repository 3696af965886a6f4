"""The numpy restatement of csrc/swd.hip in np.longdouble, and the bounds the tests hold the kernel to.

Per direction l the rows of X (n_x, F) and Y (n_y, F) are projected (longdouble dot products of the fp32 values with the float64
direction; axis mode: the value itself), both lists are sorted, and with N = n_x n_y
  W_p^p = (1 / N) sum over the cells of the common grid of 1 / N of len |x_(i) - y_(j)|^p      (p = 1: w[l, 0]; p = 2: w[l, 1])
  ks    = max over the pooled values t of |n_y #{x <= t} - n_x #{y <= t}|                      (integers: D = ks / N)
x_(i) covers the grid positions [i n_y, (i + 1) n_y) and y_(j) covers [j n_x, (j + 1) n_x); the cells are the pieces between
neighbouring breakpoints of either list, `len` their integer length.

The bounds.  u = 2^-53.  A float64 projection of row r on direction l is a sum of F products: whatever the order (the MFMA's
four at a time, a BLAS's blocks), its error is at most (F + 4) u sum_f |x_rf| |theta_lf| -- F - 1 additions and F products,
each one rounding of a partial sum no larger than sum |x| |theta| (1 + F u), and room for the fused steps' own rounding; so
with  e_l = (F + 4) u max_r sum_f |x_rf| |theta_lf|  over the rows of both sets every projection is within e_l.  Sorting is
1-Lipschitz in the maximum norm: the i-th smallest of values moved by at most e_l moves by at most e_l.  Hence every
|x_(i) - y_(j)| moves by at most 2 e_l, and as the weights len / N add up to one
  |dW_1|   <= 2 e_l                                   + s u W_1
  |dW_2^2| <= 4 e_l W_1 + 4 e_l^2                     + s u W_2^2         (|a^2 - b^2| <= 2 |a - b| b + |a - b|^2, averaged)
where the last term is the arithmetic after the sort: a term len |d|^p takes at most three roundings, the sum has at most
n_x + n_y - 1 terms, all of one sign, added in some order (at most one rounding per term, relative to the total), and one
division: s = n_x + n_y + 8 roundings relative to the result.  In axis mode the projection is exact: e_l = 0.

KS is an integer and is compared for EQUALITY.  It is a function of the order of the pooled projections alone, so it is the
same on both routes when no two pooled projections of a direction that differ at all are within 2 e_l of each other; the
tests ask for twice that (`gap_ok`: every two pooled projections are exactly equal -- duplicated rows, ties of axis mode --
or more than 4 e_l apart), from this restatement alone, before any comparison."""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def draw(F, L, seed):
    """ops.swd_draw's recipe"""
    g = np.random.RandomState(seed).standard_normal((int(L), int(F)))
    return g / np.sqrt((g * g).sum(1, keepdims=True))


def data(n_x, n_y, F, seed=0):
    """X ~ N(0, 1), Y ~ 0.7 N(0, 1) + 0.3, fp32, X drawn first"""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((n_x, F)).astype(np.float32)
    Y = (0.7 * rs.standard_normal((n_y, F)) + 0.3).astype(np.float32)
    return X, Y


def project(X, dirs, dtype=LD):
    """(L, n) projections; dirs None: axis mode"""
    if dirs is None:
        return np.ascontiguousarray(X.T).astype(dtype)
    return np.asarray(dirs).astype(dtype) @ X.astype(dtype).T


def grid_walk(xs, ys, dtype=LD):
    """(W_1, W_2^2) of two SORTED lists on the common grid of 1 / (n_x n_y)"""
    n_x, n_y = len(xs), len(ys)
    cuts = np.union1d(np.arange(n_x + 1, dtype=np.int64) * n_y, np.arange(n_y + 1, dtype=np.int64) * n_x)
    length = np.diff(cuts).astype(dtype)
    d = np.abs(xs[cuts[:-1] // n_y].astype(dtype) - ys[cuts[:-1] // n_x].astype(dtype))
    N = dtype(n_x) * dtype(n_y)
    return (length * d).sum() / N, (length * (d * d)).sum() / N


def ks_numerator(xs, ys):
    """max_t |n_y #{x <= t} - n_x #{y <= t}| over the pooled values of two SORTED lists, a Python int"""
    pooled = np.unique(np.concatenate([xs, ys]))
    cx = np.searchsorted(xs, pooled, side="right").astype(np.int64)
    cy = np.searchsorted(ys, pooled, side="right").astype(np.int64)
    return int(np.abs(len(ys) * cx - len(xs) * cy).max())


def restate(X, Y, dirs=None, dtype=LD):
    """-> {"w" (L, 2) dtype, "ks" (L,) int64, "px" (L, n_x), "py" (L, n_y): the sorted projections}"""
    px, py = np.sort(project(X, dirs, dtype), axis=1), np.sort(project(Y, dirs, dtype), axis=1)
    L = px.shape[0]
    w, ks = np.zeros((L, 2), dtype), np.zeros(L, np.int64)
    for l in range(L):
        w[l] = grid_walk(px[l], py[l], dtype)
        ks[l] = ks_numerator(px[l], py[l])
    return {"w": w, "ks": ks, "px": px, "py": py}


def projection_bound(X, Y, dirs):
    """e_l (L,) float64; zeros in axis mode"""
    if dirs is None:
        return np.zeros(X.shape[1])
    A = np.abs(np.asarray(dirs, np.float64))
    m = np.maximum((A @ np.abs(X.astype(np.float64)).T).max(1), (A @ np.abs(Y.astype(np.float64)).T).max(1))
    return (X.shape[1] + 4) * U * m * (1.0 + 1e-12)


def bounds(X, Y, dirs, ref):
    """(|dW_1| (L,), |dW_2^2| (L,), e_l (L,)) in float64 from the longdouble restatement `ref`"""
    e = projection_bound(X, Y, dirs)
    s = len(X) + len(Y) + 8
    w1, w2 = ref["w"][:, 0].astype(np.float64), ref["w"][:, 1].astype(np.float64)
    return 2 * e + s * U * w1, 4 * e * w1 + 4 * e * e + s * U * w2, e


def smallest_gap(ref, e):
    """per direction the smallest difference of two pooled projections that differ at all (inf without one), as float64, and
    whether every such difference exceeds 4 e_l"""
    gaps = np.full(len(e), np.inf)
    for l in range(len(e)):
        d = np.diff(np.sort(np.concatenate([ref["px"][l], ref["py"][l]])))
        d = d[d != 0]
        if d.size:
            gaps[l] = float(d.min())
    return gaps, bool(np.all(gaps > 4 * e))


class Case:
    def __init__(self, X, Y, dirs):
        self.X, self.Y, self.dirs = X, Y, dirs
        self.n_x, self.n_y, self.F = len(X), len(Y), X.shape[1]
        self.L = self.F if dirs is None else len(dirs)
        self.ref = restate(X, Y, dirs, LD)
        self.b1, self.b2, self.e = bounds(X, Y, dirs, self.ref)
        self.gaps, self.gap_ok = smallest_gap(self.ref, self.e)
        for a in (X, Y, dirs, self.ref["w"], self.ref["ks"]):
            if a is not None:
                a.setflags(write=False)

    def errors(self, w):
        """(|w[:, 0] - W_1|, |w[:, 1] - W_2^2|) as float64"""
        d = np.abs(np.asarray(w).astype(LD) - self.ref["w"]).astype(np.float64)
        return d[:, 0], d[:, 1]

    def held(self, w, ks):
        """every entry of w inside its bound and ks equal -> the largest errors as fractions of their bounds"""
        assert self.gap_ok, "two pooled projections of this case are nearly tied: ks cannot be compared for equality"
        e1, e2 = self.errors(w)
        assert np.all(np.isfinite(np.asarray(w, np.float64)))
        assert np.all(e1 <= self.b1), ("W_1", float(np.max(e1 / np.maximum(self.b1, 1e-300))))
        assert np.all(e2 <= self.b2), ("W_2^2", float(np.max(e2 / np.maximum(self.b2, 1e-300))))
        assert np.array_equal(np.asarray(ks, np.int64), self.ref["ks"]), "ks"
        with np.errstate(invalid="ignore", divide="ignore"):
            f1, f2 = np.where(self.b1 > 0, e1 / self.b1, 0.0), np.where(self.b2 > 0, e2 / self.b2, 0.0)
        return float(f1.max()), float(f2.max())


# (n_x, n_y, F, L) of the GPU tests
SHAPES = ((1, 1, 1, 1), (7, 5, 3, 4), (64, 64, 8, 16), (65, 63, 8, 16), (257, 130, 33, 16), (300, 211, 256, 8),
          (1000, 1024, 5, 32), (16, 16, 12288, 3), (8192, 8192, 2, 2))


@functools.lru_cache(maxsize=None)
def case(n_x, n_y, F, L, axis=False, seed=0):
    X, Y = data(n_x, n_y, F, seed)
    return Case(X, Y, None if axis else draw(F, L, seed))


@functools.lru_cache(maxsize=None)
def ties_case(axis=True):
    """integer values in {-2 .. 2} with -0.0 among +0.0, a constant column, 150 against 90 rows of 6 columns; drawn
    directions (axis False): real rows, one duplicated inside X and copied into Y twice"""
    rs = np.random.RandomState(4)
    if axis:
        X = rs.randint(-2, 3, (150, 6)).astype(np.float32)
        Y = rs.randint(-2, 3, (90, 6)).astype(np.float32)
        X[:, 5], Y[:, 5] = 1.0, 1.0
        X[::3][X[::3] == 0] = -0.0
        Y[1::2][Y[1::2] == 0] = -0.0
        return Case(X, Y, None)
    X, Y = data(70, 45, 6, 4)
    X[11], X[40], Y[7], Y[30] = X[3], X[3], X[3], X[3]
    return Case(X, Y, draw(6, 8, 4))
