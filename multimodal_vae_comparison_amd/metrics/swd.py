"""Sliced Wasserstein distances and marginal Kolmogorov-Smirnov tests of two sets of rows (csrc/swd.hip): project on many
directions, sort every projection, compare the two sorted lists -- float64, forward only."""
import math

import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["swd_draw", "swd_slices", "ks_p_value", "sliced_wasserstein", "marginal_tests"]


def _swd_rows(who, what, X):
    return ck.rows(who, what, X, 2, "(rows, F) rows",
                   ((1, 1, H.SWD_MAX_F, f"{what} has F = {{1}} features (1 .. {H.SWD_MAX_F} are on the MI355X path)"),
                    (0, 1, H.SWD_MAX_ROWS, f"{what} has {{0}} rows (1 .. {H.SWD_MAX_ROWS} per set are on the MI355X path)")),
                   defer=True)


def swd_draw(F, L, seed):
    """the directions of a sliced distance, drawn on the host: g = numpy.random.RandomState(seed).standard_normal((L, F)),
    and direction l is g[l] / sqrt(sum_f g[l, f]^2), the norm in float64 -- uniform on the unit sphere
    -> (L, F) float64 array"""
    g = np.random.RandomState(seed).standard_normal((int(L), int(F)))
    return g / np.sqrt((g * g).sum(1, keepdims=True))


def _swd_directions(who, directions, F, device):
    """contiguous float64 (L, F) on `device` or ValueError"""
    if isinstance(directions, np.ndarray):
        directions = torch.from_numpy(np.array(directions, order="C"))      # (a copy: the array may be read-only)
    if not torch.is_tensor(directions) or directions.dim() != 2 or directions.dtype != torch.float64:
        raise ValueError(f"{who}: directions is {ck.said(directions)}; a float64 (L, F) tensor or array (None: axis mode)")
    L = directions.shape[0]
    if not 1 <= L <= H.SWD_MAX_DIRECTIONS or directions.shape[1] != F:
        raise ValueError(f"{who}: directions is {tuple(directions.shape)} (1 .. {H.SWD_MAX_DIRECTIONS} directions of the rows' "
                         f"F = {F} features)")
    ck.finite(who, "directions", directions)
    return directions.detach().to(device).contiguous()


def swd_slices(X, Y, directions=None):
    """The per-direction statistics of two sets of rows X (n_x,F), Y (n_y,F).  directions: float64 (L,F) tensor or array (they
    are used as given: swd_draw makes unit rows); None is AXIS MODE, L = F <= H.SWD_MAX_DIRECTIONS and direction d is
    coordinate d (the float itself as a double: exact).  Per direction l, with the sorted projections x_(i), y_(j), N = n_x n_y:
      w[l, 0] = W_1, w[l, 1] = W_2^2 of the two empirical measures, exact for unequal sizes (the quantile functions are steps
                on a grid of 1 / N; the sum of len_ij |x_(i) - y_(j)|^p over the overlapping cells, divided by N)
      ks[l]   = max over pooled values t of |n_y #{x <= t} - n_x #{y <= t}|, an integer: the KS statistic is D = ks / N
    -> (w (L,2) float64, ks (L,) int64) on the device.  The projections run on the fp64 MFMA (k in order, no split: their bits
    depend on the row and the direction alone), every list is sorted by one workgroup in registers and LDS, no atomics: two
    runs give the same bits, and a direction's row does not depend on L or on its place.  1 <= n_x, n_y <= H.SWD_MAX_ROWS,
    F <= H.SWD_MAX_F; the rows must be finite (checked: one read of the device)."""
    return _swd_slices("swd_slices", X, Y, directions)[:2]


def _swd_slices(who, X, Y, directions):
    X, Y = _swd_rows(who, "X", X), _swd_rows(who, "Y", Y)
    ck.same_features(who, "X has", X, "Y", Y)
    ck.same_device(who, "X is", X, "Y", Y)
    n_x, n_y, F = X.shape[0], Y.shape[0], X.shape[1]
    if directions is None:
        if F > H.SWD_MAX_DIRECTIONS:
            raise ValueError(f"{who}: axis mode (directions None) takes every one of the F = {F} features as a direction, L = "
                             f"F (1 .. {H.SWD_MAX_DIRECTIONS} are on the MI355X path); give directions")
        L = F
    else:
        directions = _swd_directions(who, directions, F, X.device)
        L = directions.shape[0]
    ck.finite(who, "X", X)
    ck.finite(who, "Y", Y)
    ck.need_gpu(who, "X is", X.device)
    ws = torch.empty(H.lib().mmvae_swd_ws_doubles(n_x, n_y, F, L), dtype=torch.float64, device=X.device)
    w = torch.empty(L, 2, dtype=torch.float64, device=X.device)
    ks = torch.empty(L, dtype=torch.int64, device=X.device)
    H.call("mmvae_swd_slices", H.ptr(X), H.ptr(Y), None if directions is None else H.ptr(directions), H.ptr(ws), H.ptr(w),
           H.ptr(ks), n_x, n_y, F, L, H.stream())
    return w, ks, directions


def ks_p_value(d, n_x, n_y):
    """the asymptotic p-value of a two-sample Kolmogorov-Smirnov statistic d = sup |F_x - F_y|, on the host in float64:
    Q(lam) = 2 sum_{j >= 1} (-1)^(j - 1) exp(-2 j^2 lam^2), lam = (sqrt(n_e) + 0.12 + 0.11 / sqrt(n_e)) d, n_e = n_x n_y /
    (n_x + n_y) (Stephens' correction of the effective size), clamped to [0, 1]; 1 for d = 0.  d: a number, an array or a
    tensor -> a float, or a float64 array of d's shape.  It assumes two independent samples of continuous values."""
    if torch.is_tensor(d):
        d = d.detach().cpu().numpy()
    d = np.asarray(d, dtype=np.float64)
    n_x, n_y = int(n_x), int(n_y)
    if n_x < 1 or n_y < 1 or not np.all((d >= 0.0) & (d <= 1.0)):
        raise ValueError(f"ks_p_value: d in [0, 1] and sizes of at least one row (n_x = {n_x}, n_y = {n_y})")
    root = math.sqrt(n_x * n_y / (n_x + n_y))
    lam = (root + 0.12 + 0.11 / root) * d
    q = np.zeros_like(d)
    for j in range(1, 101):      # (the terms fall like exp(-2 j^2 lam^2); lam below 0.04 is Q = 1 to double precision)
        q += (2.0 if j % 2 else -2.0) * np.exp(-2.0 * j * j * lam * lam)
    q = np.where(lam < 0.04, 1.0, np.clip(q, 0.0, 1.0))
    return float(q) if q.ndim == 0 else q


def _swd_scalars(w):
    return {"swd1": w[:, 0].mean(), "swd2": w[:, 1].mean().sqrt(), "max_sliced1": w[:, 0].max(),
            "max_sliced2": w[:, 1].max().sqrt()}


def sliced_wasserstein(X, Y, n_directions=128, seed=0, directions=None):
    """Sliced Wasserstein distances (Rabin et al. 2011; Bonneel et al. 2015) of rows X (n_x,F) against Y (n_y,F), and their
    max-sliced variants (Deshpande et al. 2019), over the directions swd_draw(F, n_directions, seed) or `directions` ((L,F)
    float64; `n_directions` and `seed` are then not read).  With (w, ks) = swd_slices(X, Y, directions):
    -> {"swd1": mean_l W_1, "swd2": sqrt(mean_l W_2^2), "max_sliced1": max_l W_1, "max_sliced2": sqrt(max_l W_2^2), float64
        scalars on the device; "w" (L,2), "ks" (L,) int64, "directions" (L,F) float64 on the device}
    No kernel width, no feature extractor, no moment estimate: on flattened pixels this is a distance of generated images
    from real ones that needs no classifier.  There is no permutation null here."""
    who = "sliced_wasserstein"
    if directions is None:
        if not all(torch.is_tensor(t) and t.dim() == 2 for t in (X, Y)):
            raise ValueError(f"{who}: X and Y are floating (rows, F) rows")
        n_directions = int(n_directions)
        if not 1 <= n_directions <= H.SWD_MAX_DIRECTIONS:
            raise ValueError(f"{who}: n_directions = {n_directions} (1 .. {H.SWD_MAX_DIRECTIONS} are on the MI355X path)")
        if not 1 <= X.shape[1] <= H.SWD_MAX_F:
            raise ValueError(f"{who}: X has F = {X.shape[1]} features (1 .. {H.SWD_MAX_F} are on the MI355X path)")
        directions = swd_draw(X.shape[1], n_directions, seed)
    w, ks, directions = _swd_slices(who, X, Y, directions)
    out = _swd_scalars(w)
    out.update(w=w, ks=ks, directions=directions)
    return out


def marginal_tests(X, Y):
    """Per-dimension tests of rows X (n_x,F) against Y (n_y,F): swd_slices in axis mode (F <= H.SWD_MAX_DIRECTIONS), every
    coordinate on its own, exact in float64.
    -> {"w1" (F,): W_1 of dimension d, "w2" (F,): W_2 = sqrt(w[:, 1]), "ks" (F,): the Kolmogorov-Smirnov statistic D = ks_num /
        (n_x n_y), float64 on the device; "ks_p" (F,) float64 host array: ks_p_value(D, n_x, n_y); "ks_num" (F,) int64 on the
        device; "n_x", "n_y"}
    The p-values are per dimension and uncorrected; they assume independent samples."""
    w, ks, _ = _swd_slices("marginal_tests", X, Y, None)
    n_x, n_y = X.shape[0], Y.shape[0]
    # (a tensor divisor: the quotient is the correctly rounded one, not a product with the reciprocal)
    d = ks.double() / torch.full_like(ks, n_x * n_y, dtype=torch.float64)
    return {"w1": w[:, 0], "w2": w[:, 1].sqrt(), "ks": d, "ks_p": ks_p_value(d, n_x, n_y), "ks_num": ks, "n_x": n_x,
            "n_y": n_y}
