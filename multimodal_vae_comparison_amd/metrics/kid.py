"""Kernel inception distance of feature sets (csrc/kid.hip): float64 sums of polynomial kernel values, forward only."""
import math

import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["kid_sums", "kid_draw", "kernel_inception_distance"]


def _kid_index(who, what, idx, rows, device):
    """contiguous int32 (S, m) on `device` or ValueError: an integer (S, m) tensor inside the limits, every entry in
    [0, rows) -- one min/max read on the device, before any C call: the kernel does not check"""
    sizes = (f"{what} is {{0}} subsets of m = {{1}} rows (1 .. {H.KID_MAX_SUBSETS} subsets of 2 .. {H.KID_MAX_SUBSET} rows "
             f"are on the MI355X path)")
    return ck.integers(who, what, idx, 2, "an integer (S, m) tensor, one row of row numbers per subset",
                       ((0, 1, H.KID_MAX_SUBSETS, sizes), (1, 2, H.KID_MAX_SUBSET, sizes)), device, "the features",
                       inside=(0, rows, f"holds row numbers from {{0}} to {{1}}; the set has the rows 0 .. {rows - 1}"))


def _kid_kernel(who, F, degree, gamma, coef0, chunks):
    degree = int(degree)
    if not 1 <= degree <= H.KID_MAX_DEGREE:
        raise ValueError(f"{who}: degree = {degree} (1 .. {H.KID_MAX_DEGREE} are on the MI355X path)")
    chunks = ck.chunks(who, chunks)
    gamma, coef0 = 1.0 / F if gamma is None else float(gamma), float(coef0)
    if not math.isfinite(gamma) or not math.isfinite(coef0):
        raise ValueError(f"{who}: gamma = {gamma}, coef0 = {coef0} (finite numbers)")
    return degree, gamma, coef0, chunks


def _kid_sums(who, names, X, Y, idx_x, idx_y, degree, gamma, coef0, chunks):
    """every check of kid_sums, then the C call -> (sums, the int32 index lists handed to it)"""
    (nx, ny), (nix, niy) = names
    X, Y = (ck.feature_rows(who, what, t, 1, 2 ** 31 - 1, "1 .. 2^31 - 1: the index lists are int32", defer=True)
            for what, t in ((nx, X), (ny, Y)))      # (finite values: after the comparisons of the two sets)
    ck.same_features(who, f"{nx} has", X, ny, Y)
    ck.same_device(who, f"{nx} is", X, ny, Y)
    ck.finite(who, nx, X)
    ck.finite(who, ny, Y)
    F = X.shape[1]
    degree, gamma, coef0, chunks = _kid_kernel(who, F, degree, gamma, coef0, chunks)
    if torch.is_tensor(idx_x) and torch.is_tensor(idx_y) and idx_x.shape != idx_y.shape:
        raise ValueError(f"{who}: {nix} is {tuple(idx_x.shape)}, {niy} {tuple(idx_y.shape)}; both (S, m)")
    idx_x = _kid_index(who, nix, idx_x, X.shape[0], X.device)
    idx_y = _kid_index(who, niy, idx_y, Y.shape[0], X.device)
    ck.need_gpu(who, f"{nx} is", X.device)
    S, m = idx_x.shape
    ws = torch.empty(H.lib().mmvae_kid_ws_doubles(S, m, chunks), dtype=torch.float64, device=X.device)
    sums = torch.empty(S, 3, dtype=torch.float64, device=X.device)
    H.call("mmvae_kid_sums", H.ptr(X), H.ptr(Y), H.ptr(idx_x), H.ptr(idx_y), H.ptr(ws), H.ptr(sums), X.shape[0], Y.shape[0],
           F, S, m, degree, gamma, coef0, chunks, H.stream())
    return sums, idx_x, idx_y


def kid_sums(X, Y, idx_x, idx_y, degree=3, gamma=None, coef0=1.0, chunks=0):
    """The sums behind the kernel inception distance: feature rows X (rows_x,F), Y (rows_y,F); idx_x, idx_y integer (S,m),
    per subset the rows taken from X and from Y.  With k(x, y) = (gamma x . y + coef0)^degree (gamma None: 1 / F),
    x_i = X[idx_x[s,i]], y_j = Y[idx_y[s,j]] -> (S,3) float64 = [sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j),
    sum_{i,j} k(x_i, y_j)], the diagonal of the first two left out by position in the list.  Dot products in double on the
    fp64 MFMA, the rows gathered through the lists as they are loaded; neither a gathered copy nor an m x m block is
    written.  `chunks`: how many workgroups share a row's columns (0: the default plan); two plans regroup fp64 sums
    (agreement to rounding, not bit for bit), two runs with one plan give the same bits.  Every index is checked to lie
    inside its set (one min/max read per list) before the kernel runs."""
    return _kid_sums("kid_sums", (("X", "Y"), ("idx_x", "idx_y")), X, Y, idx_x, idx_y, degree, gamma, coef0, chunks)[0]


def kid_draw(n_real, n_fake, subsets, m, seed):
    """the subsets of a kernel inception distance, drawn on the host: rs = numpy.random.RandomState(seed); for s in order
    rs.choice(n_real, m, replace=False), then rs.choice(n_fake, m, replace=False) -> two (subsets, m) int64 arrays"""
    rs = np.random.RandomState(seed)
    idx_real, idx_fake = np.empty((subsets, m), dtype=np.int64), np.empty((subsets, m), dtype=np.int64)
    for s in range(subsets):
        idx_real[s] = rs.choice(n_real, m, replace=False)
        idx_fake[s] = rs.choice(n_fake, m, replace=False)
    return idx_real, idx_fake


def kernel_inception_distance(real, fake, subsets=100, subset_size=1000, seed=0, idx=None, degree=3, gamma=None, coef0=1.0,
                              chunks=0):
    """Kernel inception distance (Binkowski et al. 2018) of generated feature rows `fake` (M,F) against `real` (N,F): the
    unbiased estimate of the squared maximum mean discrepancy under k(x, y) = (gamma x . y + coef0)^degree (gamma None:
    1 / F), over `subsets` random subsets of m = min(subset_size, N, M) rows of each set, drawn without replacement
    (kid_draw(N, M, subsets, m, seed)) or given as idx = (idx_real, idx_fake), integer (S, m):
      mmd2[s] = sxx / (m (m - 1)) + syy / (m (m - 1)) - 2 sxy / m^2,   (sxx, syy, sxy) = kid_sums(...)[s]
    -> {"kid": mean_s mmd2, "std": the standard deviation of mmd2 over the subsets (divisor S), both float64 0-d tensors
        on the device, "mmd2": (S,), "sums": (S,3), "idx_real", "idx_fake": (S,m) int32 on the device, "m": m}.
    The estimator is unbiased: a negative mmd2 (and kid) is a legitimate value and is not clamped."""
    who = "kernel_inception_distance"
    if idx is None:
        if not all(torch.is_tensor(t) and t.dim() == 2 for t in (real, fake)):
            raise ValueError(f"{who}: real and fake are floating (rows, F) features")
        subsets, m = int(subsets), min(int(subset_size), real.shape[0], fake.shape[0])
        if m < 2:
            raise ValueError(f"{who}: m = min(subset_size = {subset_size}, {real.shape[0]} real rows, {fake.shape[0]} "
                             f"generated rows) = {m} (the unbiased estimate needs two rows of each set)")
        if not 1 <= subsets <= H.KID_MAX_SUBSETS or m > H.KID_MAX_SUBSET:
            raise ValueError(f"{who}: {subsets} subsets of m = {m} rows (1 .. {H.KID_MAX_SUBSETS} subsets of 2 .. "
                             f"{H.KID_MAX_SUBSET} rows are on the MI355X path)")
        idx = tuple(torch.from_numpy(i).to(device=real.device, dtype=torch.int32)
                    for i in kid_draw(real.shape[0], fake.shape[0], subsets, m, seed))
    elif not isinstance(idx, (tuple, list)) or len(idx) != 2:
        raise ValueError(f"{who}: idx is (idx_real, idx_fake), two integer (S, m) tensors")
    sums, idx_real, idx_fake = _kid_sums(who, (("real", "fake"), ("idx_real", "idx_fake")), real, fake, idx[0], idx[1],
                                         degree, gamma, coef0, chunks)
    m = idx_real.shape[1]
    mmd2 = sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)
    return {"kid": mmd2.mean(), "std": mmd2.std(unbiased=False), "mmd2": mmd2, "sums": sums, "idx_real": idx_real,
            "idx_fake": idx_fake, "m": m}
