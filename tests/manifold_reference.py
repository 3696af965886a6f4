"""Float64 restatement of the k-nearest-neighbour manifold estimates: improved precision and recall
(Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020).  Squared distances are DIRECT differences, sum_f
(x_f - y_f)^2 in double, so nothing here shares the kernels' Gram route (|x|^2 + |y|^2 - 2 x . y); the k-th neighbour
leaves the row itself out by index; every comparison is `<=`.  Also the seeded feature generator of the GPU tests and the
timing tool, the rounding bar of a Gram-route distance, and the margin between the distances and the radii they are
compared with (what makes exact equality of the counts a fair demand)."""
import functools

import numpy as np

U = 2.0 ** -53
# (N, M, F, k, shift, scale of the generated set): ragged row and column tiles, fewer rows than a tile, F no multiple of 4
# or 16, the longest F loop, more than one column chunk (and more than one tile in a chunk), k = 1, a large cheap k
SHAPES = ((9, 6, 5, 1, 0.15, 0.9), (70, 45, 50, 3, 0.15, 0.9), (130, 200, 130, 5, 0.1, 0.95), (70, 45, 2048, 5, 0.02, 1.0),
          (300, 300, 512, 5, 0.03, 1.0), (1100, 900, 64, 8, 0.15, 0.9))
# the hand-checkable integer case (k = 1): a duplicate across the sets, several distances exactly on a sphere
INT_REAL = np.array([[0, 0], [2, 0], [0, 2], [2, 2], [5, 5]], dtype=np.float32)
INT_FAKE = np.array([[1, 0], [2, 0], [4, 2], [9, 9], [0, 4]], dtype=np.float32)


def features(N, F, seed, shift=0.0, scale=1.0):
    """seeded relu features, fp32 (N, F); real sets: seed 1, shift 0, scale 1; generated sets: seed 2"""
    W = np.random.RandomState(7).standard_normal((F, F)) / np.sqrt(F)
    X = (shift + scale * np.random.RandomState(seed).standard_normal((N, F))) @ W + 0.25
    return np.maximum(X, 0.0).astype(np.float32)


def sets(N, M, F, shift, scale):
    return features(N, F, 1), features(M, F, 2, shift, scale)


def sqnorms(X):
    return (X.astype(np.float64) ** 2).sum(1)


def sqdist(B, A, block=64):
    """(len(B), len(A)) float64: sum_f (b_f - a_f)^2, in row blocks (the (block, len(A), F) temporary)"""
    B, A = B.astype(np.float64), A.astype(np.float64)
    out = np.empty((len(B), len(A)))
    for lo in range(0, len(B), block):
        d = B[lo:lo + block, None, :] - A[None, :, :]
        out[lo:lo + block] = np.einsum("ijf,ijf->ij", d, d)
    return out


def radii(X, k, D=None):
    """rad^2[i] = the k-th smallest d^2(X_i, X_j) over j != i (by index: a duplicate row is a neighbour at 0)"""
    D = sqdist(X, X) if D is None else D
    assert len(X) >= k + 1
    off = D[~np.eye(len(X), dtype=bool)].reshape(len(X), len(X) - 1)
    return np.sort(off, axis=1)[:, k - 1]


def cross(B, A, rad2, D=None):
    """(count (len(B),) int64, mind2 (len(B),)): the manifold rows whose sphere holds the query; its nearest d^2"""
    D = sqdist(B, A) if D is None else D
    return (D <= rad2[None, :]).sum(1), D.min(1)


def prdc(R, G, k):
    """every per-row quantity and the four scalars, plus `margin` = the smallest |d^2 - rad^2| over all the comparisons
    made (both orientations, coverage's included) and `scale` = max_i |x_i|^2 over both sets"""
    Drr, Dgg, Dgr = sqdist(R, R), sqdist(G, G), sqdist(G, R)
    rad_r, rad_g = radii(R, k, Drr), radii(G, k, Dgg)
    hit_r, _ = cross(G, R, rad_r, Dgr)
    hit_g, near_r = cross(R, G, rad_g, Dgr.T)
    N, M = len(R), len(G)
    margin = min(np.abs(Dgr - rad_r[None, :]).min(), np.abs(Dgr.T - rad_g[None, :]).min(), np.abs(near_r - rad_r).min())
    return {"precision": int((hit_r > 0).sum()) / M, "recall": int((hit_g > 0).sum()) / N,
            "density": int(hit_r.sum()) / (k * M), "coverage": int((near_r <= rad_r).sum()) / N,
            "hit_real": hit_r, "hit_fake": hit_g, "near_real": near_r, "rad2_real": rad_r, "rad2_fake": rad_g,
            "margin": float(margin), "scale": float(max(sqnorms(R).max(), sqnorms(G).max()))}


def bar(F, scale):
    """rounding bound of a Gram-route d^2 (and of |x|^2) in double: 8 F 2^-53 max_i |x_i|^2 -- an F-term sum of products
    bounded by max |x|^2 (Cauchy-Schwarz) carries at most F u of it, d^2 holds two norms and twice the product"""
    return 8 * F * U * scale


SCALARS = ("precision", "recall", "density", "coverage")


@functools.lru_cache(maxsize=None)
def case(i):
    """shape i of SHAPES -> (R, G, k, prdc(R, G, k)), computed once and shared (treat as read-only)"""
    N, M, F, k, shift, scale = SHAPES[i]
    R, G = sets(N, M, F, shift, scale)
    R.setflags(write=False)
    G.setflags(write=False)
    return R, G, k, prdc(R, G, k)
