"""Aggregate posterior, ELBO decomposition and mutual information gap (csrc/aggpost.hip): float64, forward only."""
import math

import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["aggregate_posterior", "elbo_decomposition", "mutual_information_gap"]


def _aggpost_rows(who, what, X, like=None):
    """contiguous fp32 (N, D) or ValueError: shape, dtype, the limits, the shape and device of `like`, finite values"""
    sizes = (f"{what} is {{0}} x {{1}} (1 .. {H.AGGPOST_MAX_ROWS} rows of 1 .. {H.AGGPOST_MAX_DIM} dimensions are on the "
             f"MI355X path)")
    return ck.rows(who, what, X, 2, "(N, D)", ((0, 1, H.AGGPOST_MAX_ROWS, sizes), (1, 1, H.AGGPOST_MAX_DIM, sizes)),
                   None if like is None else ("z", like), strict=True)


def _aggpost_labels(who, labels, N, device):
    """contiguous int32 (K, N) on `device` or ValueError: an integer (K, N) tensor, 1 <= K <= the limit, labels >= 0"""
    sizes = f"labels is {{shape}}; (K, {N}) with 1 <= K <= {H.AGGPOST_MAX_FACTORS} factors"
    return ck.integers(who, "labels", labels, 2, "an integer (K, N) tensor, one row per generative factor",
                       ((0, 1, H.AGGPOST_MAX_FACTORS, sizes), (1, N, N, sizes)), device, "z", strict=True,
                       inside=(0, 2 ** 31, "holds values outside [0, 2^31) (classes are numbered from 0)"))


def aggregate_posterior(z, loc, scale, laplace=False, labels=None, chunks=0):
    """The aggregate posterior q(z) = (1/N) sum_m q(z | x_m) at every sample: z, loc, scale (N,D), row n of z a draw from
    posterior n = Normal | Laplace (`laplace`) (loc_n, scale_n); labels (K,N) integers >= 0, one row per generative factor,
    or None.  With l[n,m,d] = log q(z_nd | x_m) in double from the fp32 inputs:
      joint (N,)              log q(z_n)  = logsumexp_m sum_d l[n,m,d] - log N
      marginal (N,D)          log q(z_nd) = logsumexp_m l[n,m,d] - log N
      conditional (K,N,D)     logsumexp over the m that share factor k's value with n of l[n,m,d] - log(class size); None
                              without labels
      self (N,)               sum_d l[n,n,d] = log q(z_n | x_n)       (torch float64 on the device)
    float64; the N x N x D terms are never written.  `chunks`: how many workgroups share a row's posterior rows (0: the
    default plan); two plans regroup fp64 sums (agreement to rounding, not bit for bit), two runs with one plan give the
    same bits.  A z that lies so far from its own posterior that exp overflows raises FloatingPointError."""
    who = "aggregate_posterior"
    chunks = ck.chunks(who, chunks, "chunks")
    z = _aggpost_rows(who, "z", z)
    loc, scale = _aggpost_rows(who, "loc", loc, z), _aggpost_rows(who, "scale", scale, z)
    if not bool((scale > 0).all()):
        raise ValueError(f"{who}: scale holds values that are not positive")
    N, D = z.shape
    lab = None if labels is None else _aggpost_labels(who, labels, N, z.device)
    K, laplace = 0 if lab is None else lab.shape[0], bool(laplace)
    ck.need_gpu(who, "z is", z.device)
    ws = torch.empty(H.lib().mmvae_aggpost_ws_doubles(N, D, K, chunks), dtype=torch.float64, device=z.device)
    joint = torch.empty(N, dtype=torch.float64, device=z.device)
    marginal = torch.empty(N, D, dtype=torch.float64, device=z.device)
    cond = None if lab is None else torch.empty(K, N, D, dtype=torch.float64, device=z.device)
    H.call("mmvae_aggpost_lse", H.ptr(z), H.ptr(loc), H.ptr(scale), int(laplace), H.ptr(lab), H.ptr(ws), H.ptr(joint),
           H.ptr(marginal), H.ptr(cond), N, D, K, chunks, H.stream())
    s = scale.double()
    t = (z.double() - loc.double()) / s
    own = (-t.abs() - torch.log(2.0 * s)) if laplace else (-0.5 * t * t - torch.log(s) - 0.5 * math.log(2.0 * math.pi))
    if not bool(torch.isfinite(joint).all()) or not bool(torch.isfinite(marginal).all()):
        raise FloatingPointError(f"{who}: a row of z lies so far from its own posterior that exp(l - l[n,n]) overflows "
                                 f"(z must be a draw from the posterior of its row)")
    return {"joint": joint, "marginal": marginal, "conditional": cond, "self": own.sum(1)}


_AGG_KEYS = ("joint", "marginal", "conditional", "self")


def _aggpost_result(who, agg):
    """the (joint, marginal, conditional, self) of an aggregate_posterior result or ValueError"""
    if not isinstance(agg, dict) or any(k not in agg for k in _AGG_KEYS):
        raise ValueError(f"{who}: agg must be the dict aggregate_posterior returns ({', '.join(_AGG_KEYS)})")
    joint, marginal, cond, own = (agg[k] for k in _AGG_KEYS)
    for what, t, dims in (("joint", joint, 1), ("marginal", marginal, 2), ("self", own, 1)):
        if not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != dims:
            raise ValueError(f"{who}: agg[{what!r}] must be a float64 tensor of {dims} dimension(s)")
    N, D = marginal.shape
    if joint.shape != (N,) or own.shape != (N,) or N < 1 or D < 1:
        raise ValueError(f"{who}: agg holds joint {tuple(joint.shape)}, self {tuple(own.shape)}, marginal {(N, D)}")
    if cond is not None and (not torch.is_tensor(cond) or cond.dtype != torch.float64 or cond.dim() != 3
                             or cond.shape[1:] != (N, D)):
        raise ValueError(f"{who}: agg['conditional'] must be None or float64 (K, {N}, {D})")
    return joint, marginal, cond, own


def elbo_decomposition(agg, lpz):
    """The decomposition of the ELBO's KL term (Chen et al. 2018) from an aggregate_posterior result and lpz (N,) = sum_d
    log p(z_nd) under the prior:
      mi   = mean_n(log q(z_n | x_n) - log q(z_n))         index-code mutual information
      tc   = mean_n(log q(z_n) - sum_d log q(z_nd))        total correlation
      dwkl = mean_n(sum_d log q(z_nd) - log p(z_n))        dimension-wise KL
      kl   = mean_n(log q(z_n | x_n) - log p(z_n))         = mi + tc + dwkl
    -> 0-d float64 tensors on the device."""
    who = "elbo_decomposition"
    joint, marginal, _, own = _aggpost_result(who, agg)
    if not torch.is_tensor(lpz) or lpz.shape != joint.shape or not lpz.is_floating_point():
        raise ValueError(f"{who}: lpz is {ck.said(lpz)}; floating ({joint.shape[0]},), the prior's log-density of every row "
                         f"of z")
    ck.same_device(who, "lpz is", lpz, "agg", joint)
    lpz = lpz.detach().double()
    ck.finite(who, "lpz", lpz)
    sum_marginal = marginal.sum(1)
    return {"mi": (own - joint).mean(), "tc": (joint - sum_marginal).mean(), "dwkl": (sum_marginal - lpz).mean(),
            "kl": (own - lpz).mean()}


def mutual_information_gap(agg, labels):
    """The mutual information gap (Chen et al. 2018) from an aggregate_posterior result that was given `labels` (K,N):
      h_z (D,)         H(z_d) = -mean_n log q(z_nd)
      mi (K,D)         I(z_d; v_k) = H(z_d) - H(z_d | v_k), H(z_d | v_k) = -mean_n conditional[k,n,d] (the mean over all n
                       weights every class by its frequency)
      h_v (K,)         H(v_k) from the class counts
      per_factor (K,)  (largest - second largest of mi[k,:]) / H(v_k);  mig = their mean
    float64 on the device.  D >= 2, and every factor must take at least two values (H(v_k) > 0)."""
    who = "mutual_information_gap"
    _, marginal, cond, _ = _aggpost_result(who, agg)
    if cond is None:
        raise ValueError(f"{who}: agg holds no conditional (aggregate_posterior was called without labels)")
    N, D = marginal.shape
    lab = _aggpost_labels(who, labels, N, marginal.device)
    if lab.shape[0] != cond.shape[0]:
        raise ValueError(f"{who}: labels has {lab.shape[0]} factors, agg['conditional'] {cond.shape[0]}")
    if D < 2:
        raise ValueError(f"{who}: D = {D} latent dimension (the gap is between the two most informative dimensions)")
    h_v = []
    for k in range(lab.shape[0]):
        p = torch.bincount(lab[k].long()).double() / N
        p = p[p > 0]
        if p.numel() < 2:
            raise ValueError(f"{who}: factor {k} of labels takes a single value (H(v) = 0: the gap is not defined)")
        h_v.append(-(p * p.log()).sum())
    h_v = torch.stack(h_v)
    h_z = -marginal.mean(0)
    mi = h_z.unsqueeze(0) + cond.mean(1)
    top = mi.topk(2, dim=1).values
    per = (top[:, 0] - top[:, 1]) / h_v
    return {"mig": per.mean(), "per_factor": per, "mi": mi, "h_z": h_z, "h_v": h_v}
