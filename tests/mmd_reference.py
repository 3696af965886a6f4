"""Numpy restatement of the kernel two-sample test (csrc/mmd.hip) by direct differences, written
once and run in float64 and in numpy.longdouble, the recipe of ops.mmd_draw, the p-value, and the case table that
tests/test_mmd_host.py and tests/test_mmd_gpu.py share.  Nothing here imports the package.

The bound of an entry of `sums` or `row_sums` (the issue's): 16 x the error the float64 restatement itself shows against
the longdouble one on that case, at least 1e-13 x the sum of |k_ij| over the entry's terms.  The factor covers another
order of summation and the tile form, measured from a reference that carries the same kind of rounding."""
import functools

import numpy as np

LD = np.longdouble
PBLOCK = 128                     # hipops.MMD_PBLOCK (the host test holds the two equal)
EXTRA = 1                        # hipops.MMD_EXTRA_COLUMNS: the observed split rides in the first block of columns
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
FACTOR, FLOOR, APART = 16.0, 1e-13, 1000.0


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def sqdist(Z, dtype):
    """(n, n) squared distances by direct differences, features in order"""
    Z = np.asarray(Z).astype(dtype)
    d2 = np.zeros((len(Z), len(Z)), dtype)
    for f in range(Z.shape[1]):
        diff = Z[:, f][:, None] - Z[:, f][None, :]
        d2 += diff * diff
    return d2


def kernel_of(d2, kernel, params, dtype):
    """the kernel function of a matrix of squared distances"""
    if kernel == "energy":
        return -np.sqrt(d2)
    out = np.zeros_like(d2)
    for p in params:
        p = dtype(p)
        out += np.exp(-p * d2) if kernel == "rbf" else p / (p + d2)
    return out / dtype(len(params))


def auto_params(Z, kernel, scales=SCALES):
    """the automatic widths: m2 = 2 n / (n - 1) sum_d var_d (biased variances, float64)"""
    if kernel == "energy":
        return ()
    Z = np.asarray(Z, np.float64)
    n = len(Z)
    m2 = 2.0 * n / (n - 1) * float(Z.var(0).sum())
    return tuple(1.0 / (s * m2) for s in scales) if kernel == "rbf" else tuple(s * m2 for s in scales)


def splits(n_x, n_y, member):
    """(1 + P, n) 0 / 1: the observed split, then the relabellings"""
    first = np.concatenate([np.ones(n_x, np.uint8), np.zeros(n_y, np.uint8)])[None]
    return first if member is None or len(member) == 0 else np.concatenate([first, np.asarray(member, np.uint8)])


def sums_of(K, A):
    """K (n, n) with a zero diagonal, A (R, n) 0 / 1 -> (R, 3) = [both X, both Y, X against Y], each added up directly"""
    A = A.astype(K.dtype)
    B = 1 - A
    AK, BK = A @ K, B @ K
    return np.stack([(AK * A).sum(1), (BK * B).sum(1), (AK * B).sum(1)], 1)


def restate(X, Y, member, kernel, params, dtype, keep_diagonal=False, root_in_rbf=False, swap=False):
    """-> {"K", "sums" (1 + P, 3), "row_sums" (n,), "abs_sums", "abs_rows": the same sums of |k_ij|}.  The three
    keywords are the seeded errors of the host test: the diagonal kept, gamma applied to d instead of d^2, the groups
    swapped."""
    Z = np.concatenate([X, Y])
    d2 = sqdist(Z, dtype)
    K = kernel_of(np.sqrt(d2) if root_in_rbf else d2, kernel, params, dtype)
    if not keep_diagonal:
        np.fill_diagonal(K, 0)
    A = splits(len(X), len(Y), member)
    if swap:
        A = 1 - A
    return {"K": K, "sums": sums_of(K, A), "row_sums": K.sum(1), "abs_sums": sums_of(np.abs(K), A),
            "abs_rows": np.abs(K).sum(1)}


def mmd2_of(sums, n_x, n_y, divisor_bug=False):
    """the unbiased estimate of every row of sums (`divisor_bug`: the seeded error n^2 for n (n - 1))"""
    dx, dy = (n_x * n_x, n_y * n_y) if divisor_bug else (n_x * (n_x - 1), n_y * (n_y - 1))
    return sums[..., 0] / dx + sums[..., 1] / dy - 2 * sums[..., 2] / (n_x * n_y)


def draw(n_x, n_y, permutations, seed):
    """ops.mmd_draw's documented recipe"""
    rs = np.random.RandomState(seed)
    member = np.zeros((permutations, n_x + n_y), np.uint8)
    for p in range(permutations):
        member[p, rs.permutation(n_x + n_y)[:n_x]] = 1
    return member


def p_value(mmd2, null):
    return (1 + int(np.sum(np.asarray(null) >= mmd2))) / (1 + len(null))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _same(rs, n_x, n_y, D):
    return rs.randn(n_x, D), rs.randn(n_y, D)


def _shifted(rs, n_x, n_y, D):
    return rs.randn(n_x, D), rs.randn(n_y, D) + 1.0      # the mean moved by one standard deviation


def _dup(rs, n_x, n_y, D):
    Z = rs.randn(n_x + n_y, D)
    where = [0, 3, n_x // 2, n_x - 2, n_x - 1, n_x, n_x + 1, n_x + n_y // 2, n_x + n_y - 2, n_x + n_y - 1]
    Z[where] = Z[where[0]]      # ten identical rows spread over both sets
    return Z[:n_x], Z[n_x:]


def _offset(rs, n_x, n_y, D):
    return 1000.0 + 0.01 * rs.randn(n_x, D), 1000.0 + 0.01 * rs.randn(n_y, D) + 0.003


def _far(rs, n_x, n_y, D):
    """two clusters of unit width 50 apart, both in both sets: with the widths 1 and 2 every term between the clusters
    underflows to 0 in double (exp(-1250) and less)"""
    Z = rs.randn(n_x + n_y, D)
    Z[::2, 0] += 50.0
    return Z[:n_x], Z[n_x:]


DATA = {"same": _same, "shifted": _shifted, "dup": _dup, "offset": _offset, "far": _far}

# name: (data, n_x, n_y, D, P, kernel, params | None: automatic, scales, seed of the rows, seed of the relabellings)
S1, S8 = (1.0,), (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
CASES = {
    "2x2": ("same", 2, 2, 3, 3, "rbf", None, SCALES, 1, 7),      # (seed 7: no relabelling is the observed split or its mirror)
    "63x65-D31-P1-imq": ("same", 63, 65, 31, 1, "imq", None, SCALES, 2, 0),
    "64x64-D32-Pblock-1": ("same", 64, 64, 32, PBLOCK - EXTRA - 1, "rbf", None, SCALES, 3, 0),
    "65x128-D33-Pblock-energy": ("same", 65, 128, 33, PBLOCK - EXTRA, "energy", None, SCALES, 4, 0),
    "n127-D8-Pblock+1-S1": ("same", 60, 67, 8, PBLOCK - EXTRA + 1, "rbf", None, S1, 5, 0),
    "n129-D1-S8": ("shifted", 64, 65, 1, 5, "rbf", None, S8, 6, 0),
    "n191-D16-P0-imq": ("same", 100, 91, 16, 0, "imq", None, SCALES, 7, 0),
    "n193-D256": ("same", 96, 97, 256, 4, "rbf", None, SCALES, 8, 0),
    "n255-D5-energy": ("shifted", 128, 127, 5, 7, "energy", None, SCALES, 9, 0),
    "n257-D40-imq-S8": ("same", 128, 129, 40, PBLOCK + 1, "imq", None, S8, 10, 0),
    "n300-D8": ("same", 150, 150, 8, 20, "rbf", None, SCALES, 11, 0),
    "dup-rbf": ("dup", 40, 41, 6, 20, "rbf", None, SCALES, 12, 0),
    "dup-imq": ("dup", 40, 41, 6, 20, "imq", None, SCALES, 12, 0),
    "dup-energy": ("dup", 40, 41, 6, 20, "energy", None, SCALES, 12, 0),
    "offset-rbf": ("offset", 70, 60, 12, 20, "rbf", None, SCALES, 13, 0),
    "offset-imq": ("offset", 70, 60, 12, 20, "imq", None, SCALES, 13, 0),
    "offset-energy": ("offset", 70, 60, 12, 20, "energy", None, SCALES, 13, 0),
    "far": ("far", 50, 50, 4, 20, "rbf", (1.0, 0.5), None, 14, 0),
    "same": ("same", 100, 100, 8, 199, "rbf", None, SCALES, 15, 0),
    "shifted": ("shifted", 100, 100, 8, 199, "rbf", None, SCALES, 16, 0),
}
NAMES = list(CASES)
# chunk plans beside the default one: a single chunk and one chunk per column tile
PLANS = {"n300-D8": (1, 5), "65x128-D33-Pblock-energy": (1, 4), "n129-D1-S8": (1, 3)}


class Case:
    def __init__(self, name):
        data, self.n_x, self.n_y, self.D, self.P, self.kernel, params, self.scales, seed, self.draw_seed = CASES[name]
        self.name, self.n = name, self.n_x + self.n_y
        X, Y = DATA[data](np.random.RandomState(seed), self.n_x, self.n_y, self.D)
        self.X, self.Y = X.astype(np.float32), Y.astype(np.float32)
        self.member = draw(self.n_x, self.n_y, self.P, self.draw_seed)
        Z = np.concatenate([self.X, self.Y])
        self.params = tuple(params) if params is not None else auto_params(Z, self.kernel, self.scales)
        self.given = params is not None
        self.ld = restate(self.X, self.Y, self.member, self.kernel, self.params, LD)
        self.f64 = restate(self.X, self.Y, self.member, self.kernel, self.params, np.float64)
        self.err = {k: np.abs(self.f64[k].astype(LD) - self.ld[k]).astype(np.float64) for k in ("sums", "row_sums")}
        self.bound = {"sums": np.maximum(FACTOR * self.err["sums"], FLOOR * self.ld["abs_sums"].astype(np.float64)),
                      "row_sums": np.maximum(FACTOR * self.err["row_sums"], FLOOR * self.ld["abs_rows"].astype(np.float64))}
        for v in (self.X, self.Y, self.member):
            v.setflags(write=False)
        self.mmd2 = mmd2_of(self.ld["sums"], self.n_x, self.n_y)
        b = self.bound["sums"]
        # what the bounds of the three sums allow the estimate to move
        self.mmd2_bound = b[:, 0] / (self.n_x * (self.n_x - 1)) + b[:, 1] / (self.n_y * (self.n_y - 1)) + \
            2 * b[:, 2] / (self.n_x * self.n_y)
        self.p_value = p_value(self.mmd2[0], self.mmd2[1:])

    def apart(self):
        """the smallest |permuted - observed| over APART x (the two bounds together): > 1 means that no estimate inside
        its bound can change the count behind the p-value"""
        if not self.P:
            return np.inf
        gap = np.abs(self.mmd2[1:] - self.mmd2[0]).astype(np.float64)
        return float(np.min(gap / (APART * (self.mmd2_bound[1:] + self.mmd2_bound[0]))))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
