"""Kernel two-sample test of latent rows (csrc/mmd.hip): float64 sums of kernel values for the observed split and for
relabellings of the pooled sample, forward only."""
import ctypes
import math

import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["mmd_sums", "mmd_draw", "mmd_two_sample", "mmd2_from_sums", "MMD_SCALES"]

MMD_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)


def _mmd_rows(who, what, X):
    return ck.rows(who, what, X, 2, "(rows, D) latent rows",
                   ((1, 1, H.MMD_MAX_D, f"{what} has D = {{1}} dimensions (1 .. {H.MMD_MAX_D} are on the MI355X path)"),
                    (0, 2, H.MMD_MAX_ROWS, f"{what} has {{0}} rows (2 .. {H.MMD_MAX_ROWS}: the unbiased estimate needs two "
                                           f"rows of each set, and both sets together at most {H.MMD_MAX_ROWS})")), defer=True)


def _mmd_positive(who, what, values):
    """a tuple of 1 .. MMD_MAX_SCALES finite positive floats or ValueError"""
    try:
        values = tuple(float(v) for v in values)
    except TypeError:
        raise ValueError(f"{who}: {what} is {type(values).__name__}; a sequence of 1 .. {H.MMD_MAX_SCALES} positive "
                         f"numbers") from None
    if not 1 <= len(values) <= H.MMD_MAX_SCALES or not all(math.isfinite(v) and v > 0.0 for v in values):
        raise ValueError(f"{who}: {what} = {values} (1 .. {H.MMD_MAX_SCALES} finite positive numbers)")
    return values


def _mmd_member(who, member, n_x, n, device):
    """contiguous uint8 (P, n) on `device` or ValueError: entries 0 / 1 and n_x ones per row -- ONE read of the device (the
    four extremes travel together), before any C call: the kernel does not check"""
    if isinstance(member, np.ndarray):
        member = torch.from_numpy(np.ascontiguousarray(member)).to(device)
    sizes = (f"member is {{0}} relabellings of {{1}} pooled rows (0 .. {H.MMD_MAX_PERMUTATIONS} relabellings of n_x + n_y = "
             f"{n} rows)")
    member = ck.integers(who, "member", member, 2, "an integer (P, n) tensor or array of 0 / 1, one row per relabelling",
                         ((0, 0, H.MMD_MAX_PERMUTATIONS, sizes), (1, n, n, sizes)), device, "the rows", to=None)
    if member.shape[0]:
        ones = member.sum(1, dtype=torch.int64)
        lo, hi, least, most = (int(v) for v in torch.stack([member.amin().long(), member.amax().long(), ones.amin(),
                                                            ones.amax()]).tolist())
        if lo < 0 or hi > 1:
            raise ValueError(f"{who}: member holds values from {lo} to {hi}; 1 marks a row of the first set, 0 of the second")
        if least != n_x or most != n_x:
            raise ValueError(f"{who}: the rows of member mark {least} .. {most} pooled rows; every relabelling keeps the "
                             f"first set's size, n_x = {n_x}")
    return member.to(torch.uint8).contiguous()


def _mmd_sums(who, names, X, Y, member, kernel, params, scales, chunks):
    """every check of mmd_sums, then the C call -> (sums, row_sums, params, the uint8 member handed to it)"""
    nx, ny = names
    X, Y = _mmd_rows(who, nx, X), _mmd_rows(who, ny, Y)
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"{who}: {nx} has D = {X.shape[1]} dimensions, {ny} D = {Y.shape[1]}")
    ck.same_device(who, f"{nx} is", X, ny, Y)
    n_x, n_y, D = X.shape[0], Y.shape[0], X.shape[1]
    n = n_x + n_y
    if n > H.MMD_MAX_ROWS:
        raise ValueError(f"{who}: {nx} and {ny} have {n_x} + {n_y} = {n} rows together (at most {H.MMD_MAX_ROWS} are on the "
                         f"MI355X path)")
    ck.finite(who, nx, X)
    ck.finite(who, ny, Y)
    if kernel not in H.MMD_KERNELS:
        raise ValueError(f"{who}: kernel = {kernel!r} (one of {', '.join(H.MMD_KERNELS)})")
    chunks = ck.chunks(who, chunks)
    if kernel == "energy":
        if params is not None and len(tuple(params)):
            raise ValueError(f"{who}: the energy kernel k = -d has no parameters; params = {params}")
        params = ()
    elif params is not None:
        params = _mmd_positive(who, "params", params)
    else:
        scales = _mmd_positive(who, "scales", scales)
    member = torch.zeros(0, n, dtype=torch.uint8, device=X.device) if member is None else \
        _mmd_member(who, member, n_x, n, X.device)
    if params is None:
        # the mean squared distance of the pooled sample over i != j, in closed form: sum_{i,j} d^2 = 2 n^2 sum_d var_d
        pooled = torch.cat([X, Y]).double()
        m2 = 2.0 * n / (n - 1) * float(pooled.var(0, unbiased=False).sum())
        if not (math.isfinite(m2) and m2 > 0.0):
            raise ValueError(f"{who}: the mean squared distance of the pooled rows is {m2}; the automatic width needs rows "
                             f"that differ (or give params)")
        params = tuple(1.0 / (s * m2) for s in scales) if kernel == "rbf" else tuple(s * m2 for s in scales)
    ck.need_gpu(who, f"{nx} is", X.device)
    P = member.shape[0]
    ws = torch.empty(H.lib().mmvae_mmd_ws_doubles(n, D, P, chunks), dtype=torch.float64, device=X.device)
    sums = torch.empty(1 + P, 3, dtype=torch.float64, device=X.device)
    row_sums = torch.empty(n, dtype=torch.float64, device=X.device)
    host = (ctypes.c_double * max(len(params), 1))(*params)
    H.call("mmvae_mmd_sums", H.ptr(X), H.ptr(Y), H.ptr(member) if P else None, H.ptr(ws), H.ptr(sums), H.ptr(row_sums), n_x,
           n_y, D, P, H.MMD_KERNELS[kernel], ctypes.addressof(host), len(params), chunks, H.stream())
    return sums, row_sums, params, member


def mmd_sums(X, Y, member=None, kernel="rbf", params=None, scales=MMD_SCALES, chunks=0):
    """The sums behind a kernel two-sample test: rows X (n_x,D), Y (n_y,D); the pooled order is X's rows, then Y's, n = n_x
    + n_y.  member: integer (P,n) of 0 / 1 (tensor on the rows' device, or a host array), row p marks the pooled rows that
    count as "X" under relabelling p, n_x ones per row (None: no relabelling).  With d^2 = |x - y|^2,
      kernel "rbf"     k = (1/S) sum_s exp(-params[s] d^2)              params: the rates gamma_s
             "imq"     k = (1/S) sum_s params[s] / (params[s] + d^2)    params: the constants c_s
             "energy"  k = -d                                           no parameters
    params None: from the mean squared distance of the pooled sample over i != j, m2 = 2 n / (n - 1) sum_d var_d (biased
    variances, float64): gamma_s = 1 / (scales[s] m2), c_s = scales[s] m2 -- a function of the pooled sample alone, so
    every relabelling shares it and the permutation test stays valid.
    -> (sums (1 + P, 3) float64: row 0 the observed split, row 1 + p relabelling p, each [sum_{i != j both X} k_ij,
        sum_{i != j both Y} k_ij, sum_{i in X, j in Y} k_ij], the diagonal left out by position;
        row_sums (n,) float64: r_i = sum_{j != i} k_ij;   params: the tuple of floats the kernel used)
    Rows are centred by the pooled mean in double and the Gram tiles run on the fp64 MFMA; every tile is multiplied by a
    block of H.MMD_PBLOCK indicator columns there, and the n x n matrix is never written.  `chunks`: how many workgroups
    share a row's columns (0: the default plan, a function of n alone); two plans regroup fp64 sums (agreement to
    rounding), two runs with one plan give the same bits, and a relabelling's row does not depend on P or on its place in
    member.  member is checked (0 / 1, n_x ones per row: one read of the device) before the kernel runs."""
    return _mmd_sums("mmd_sums", ("X", "Y"), X, Y, member, kernel, params, scales, chunks)[:3]


def mmd_draw(n_x, n_y, permutations, seed):
    """the relabellings of a two-sample test, drawn on the host: rs = numpy.random.RandomState(seed); for p in order
    perm = rs.permutation(n_x + n_y), and the pooled rows perm[:n_x] are the X group of relabelling p
    -> (permutations, n_x + n_y) uint8 array, 1 on those rows"""
    n_x, n_y, permutations = int(n_x), int(n_y), int(permutations)
    rs = np.random.RandomState(seed)
    member = np.zeros((permutations, n_x + n_y), dtype=np.uint8)
    for p in range(permutations):
        member[p, rs.permutation(n_x + n_y)[:n_x]] = 1
    return member


def mmd2_from_sums(sums, n_x, n_y):
    """the unbiased MMD^2 of every row of sums (.., 3): sxx / (n_x (n_x - 1)) + syy / (n_y (n_y - 1)) - 2 sxy / (n_x n_y)"""
    return sums[..., 0] / (n_x * (n_x - 1)) + sums[..., 1] / (n_y * (n_y - 1)) - 2.0 * sums[..., 2] / (n_x * n_y)


def mmd_two_sample(X, Y, permutations=1000, seed=0, member=None, kernel="rbf", params=None, scales=MMD_SCALES, chunks=0):
    """Kernel two-sample test (Gretton et al. 2012) of rows X (n_x,D) against Y (n_y,D) with a permutation null: the
    relabellings are mmd_draw(n_x, n_y, permutations, seed), or `member` (see mmd_sums; `permutations` and `seed` are then
    not read).  kernel, params, scales, chunks: as in mmd_sums.
    -> {"mmd2": the unbiased estimate of the observed split (mmd2_from_sums of row 0; it may be negative and is not
        clamped), "null": (P,) the estimates of the relabellings, "p_value": (1 + #{null >= mmd2}) / (1 + P),
        "null_mean", "null_std" (divisor P), "z": (mmd2 - null_mean) / null_std (nan without a spread), all float64 on
        the device but p_value, a float; "sums" (1 + P, 3), "row_sums" (n,), "params": the tuple of floats used,
        "member": (P,n) uint8 on the device}"""
    who = "mmd_two_sample"
    if member is None:
        if not all(torch.is_tensor(t) and t.dim() == 2 for t in (X, Y)):
            raise ValueError(f"{who}: X and Y are floating (rows, D) latent rows")
        permutations = int(permutations)
        if not 0 <= permutations <= H.MMD_MAX_PERMUTATIONS:
            raise ValueError(f"{who}: permutations = {permutations} (0 .. {H.MMD_MAX_PERMUTATIONS} are on the MI355X path)")
        member = mmd_draw(X.shape[0], Y.shape[0], permutations, seed)
    sums, row_sums, params, member = _mmd_sums(who, ("X", "Y"), X, Y, member, kernel, params, scales, chunks)
    est = mmd2_from_sums(sums, X.shape[0], Y.shape[0])
    mmd2, null = est[0], est[1:]
    P = null.shape[0]
    nan = torch.full((), float("nan"), dtype=torch.float64, device=sums.device)
    mean = null.mean() if P else nan
    std = null.std(unbiased=False) if P else nan
    return {"mmd2": mmd2, "null": null, "p_value": (1 + int((null >= mmd2).sum())) / (1 + P), "null_mean": mean,
            "null_std": std, "z": (mmd2 - mean) / std if P else nan, "sums": sums, "row_sums": row_sums, "params": params,
            "member": member}
