"""Latent density estimation (csrc/gmm.hip): Gaussian-mixture EM, scoring, draws; float64, forward only."""
import math

import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["GMM_SLICE_BYTES", "gmm_check_init", "gmm_check_fit_args", "gmm_fit", "gmm_score", "gmm_sample", "gmm_information"]


GMM_SLICE_BYTES = 256 << 20      # restarts run in slices whose responsibilities and workspace stay under this


def _gmm_rows(who, X, D=None):
    """contiguous fp32 (N, D) rows inside the limits (and of `D` dimensions, where given) or ValueError"""
    X = ck.feature_rows(who, "X", X, 1, H.MANIFOLD_MAX_ROWS, f"1 .. {H.MANIFOLD_MAX_ROWS} are on the MI355X path", defer=True)
    if not 1 <= X.shape[1] <= H.GMM_MAX_D:
        raise ValueError(f"{who}: X has D = {X.shape[1]} dimensions (1 .. {H.GMM_MAX_D} are on the MI355X path)")
    if D is not None and X.shape[1] != D:
        raise ValueError(f"{who}: X has D = {X.shape[1]} dimensions, the mixture {D}")
    ck.finite(who, "X", X)
    return X


def _gmm_covariance(who, covariance_type):
    if covariance_type not in H.GMM_COVARIANCES:
        raise ValueError(f"{who}: covariance_type = {covariance_type!r} ({', '.join(map(repr, H.GMM_COVARIANCES))} are on "
                         f"the MI355X path)")
    return H.GMM_COVARIANCES[covariance_type]


def gmm_check_init(who, init, N, n_components=None):
    """the start of a mixture fit on N rows or ValueError: integer (R, N) labels, one per row and restart, inside
    [0, n_components) (None: the largest id + 1 components); R and the components inside the limits
    -> (init as an int32 tensor, C)"""
    init = ck.integers(who, "init", init, 2, "integer (R, N) labels, one component id per restart and row",
                       ((0, 1, H.CLUSTER_MAX_INIT, f"{{0}} restarts (1 .. {H.CLUSTER_MAX_INIT} are on the MI355X path)"),
                        (1, N, N, f"init has {{1}} labels per restart for {N} rows")), arrays=np.ndarray, to=None)
    lo, hi = ck.extremes(init)
    C = hi + 1 if n_components is None else int(n_components)
    if not 1 <= C <= H.CLUSTER_MAX_K:
        raise ValueError(f"{who}: {C} components (1 .. {H.CLUSTER_MAX_K} are on the MI355X path)")
    if lo < 0 or hi >= C:
        raise ValueError(f"{who}: init holds the ids {lo} .. {hi}; n_components = {C} has the ids 0 .. {C - 1}")
    return init.to(torch.int32).contiguous(), C


def gmm_check_fit_args(who, reg_covar, tol, max_iter):
    reg_covar, tol, max_iter = float(reg_covar), float(tol), int(max_iter)
    if not (reg_covar >= 0.0 and math.isfinite(reg_covar)):
        raise ValueError(f"{who}: reg_covar = {reg_covar} (a finite value >= 0)")
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError(f"{who}: tol = {tol} (a finite value >= 0)")
    if not 1 <= max_iter <= H.CLUSTER_MAX_ITER:
        raise ValueError(f"{who}: max_iter = {max_iter} (1 .. {H.CLUSTER_MAX_ITER} are on the MI355X path)")
    return reg_covar, tol, max_iter


def gmm_fit(X, init, covariance_type="full", reg_covar=1e-6, tol=1e-3, max_iter=100, sync_every=10, n_components=None,
            slice_bytes=None):
    """EM for a mixture of C Gaussians on the rows of X (N,D), read as double, R restarts side by side, with the arithmetic of
    scikit-learn's GaussianMixture (covariance_type "full" or "diag").  `init`: integer (R,N) labels; restart r starts from
    their one-hot as responsibilities and one M-step (C = `n_components`, or the largest id + 1; a component without rows
    starts as N(0, reg_covar I) with weight ~0).  Iteration t = 1, 2, ...: E-step, M-step; the restart has converged when the
    E-step's lower bound (the mean log-density) moved by less than `tol`; n_iter = t.  A restart one of whose covariances
    has no Cholesky factor is `degenerate` (bound -inf, never `best`); when every restart is, ValueError.  Three launches
    per iteration for all restarts; the host reads the restarts' records every `sync_every` iterations.  Restarts run in
    slices of `slice_bytes` (GMM_SLICE_BYTES) of responsibilities and workspace.
    -> {"weights" (R,C), "means" (R,C,D), "covariances" (R,C,D,D) | (R,C,D), "cholesky" (lower factors; diag: square roots),
        "precisions_cholesky", "log_det" (R,C), "lower_bound" (R,), "n_iter" (R,) int32, "converged", "degenerate" (R,) bool,
        "best": the restart of the largest bound (the lowest of equals), "labels" (R,N) int32, "resp" (R,N,C), "log_density"
        (R,N) of the final parameters, "covariance_type"}, float64.  Two runs, a restart alone or beside others, any
        `sync_every` and any slicing give the same bits."""
    who = "gmm_fit"
    X = _gmm_rows(who, X)
    N, D = X.shape
    diag = _gmm_covariance(who, covariance_type)
    reg_covar, tol, max_iter = gmm_check_fit_args(who, reg_covar, tol, max_iter)
    sync_every = int(sync_every)
    if sync_every < 1:
        raise ValueError(f"{who}: sync_every = {sync_every} (at least one iteration between two looks at the records)")
    init, C = gmm_check_init(who, init, N, n_components)
    R = init.shape[0]
    slice_bytes = GMM_SLICE_BYTES if slice_bytes is None else int(slice_bytes)
    if slice_bytes < 1:
        raise ValueError(f"{who}: slice_bytes = {slice_bytes} (a positive number of bytes; one restart runs in any case)")
    ck.need_gpu(who, "X is", X.device, "the kernels run")
    dev = X.device
    init = init.to(dev)
    per = 8 * (N * C + H.lib().mmvae_gmm_ws_doubles(N, D, C, 1, diag))
    step = max(1, min(R, slice_bytes // per))
    shape = (D,) if diag else (D, D)
    parts = []
    for r0 in range(0, R, step):
        Rs = min(step, R - r0)
        f64 = dict(dtype=torch.float64, device=dev)
        weights, logdet = torch.empty(Rs, C, **f64), torch.empty(Rs, C, **f64)
        means = torch.empty(Rs, C, D, **f64)
        cov, chol, prec = (torch.empty(Rs, C, *shape, **f64) for _ in range(3))
        resp = torch.empty(Rs, N, C, **f64)
        ws = torch.zeros(H.lib().mmvae_gmm_ws_doubles(N, D, C, Rs, diag), **f64)
        state = ws[:4 * Rs].view(Rs, 4)
        bad = ws[4 * Rs:(4 + H.CLUSTER_MAX_K) * Rs].view(Rs, H.CLUSTER_MAX_K)
        start = init[r0:r0 + Rs].contiguous()
        for it0 in range(1, max_iter + 1, sync_every):
            H.call("mmvae_gmm_em", H.ptr(X), H.ptr(start), H.ptr(weights), H.ptr(means), H.ptr(cov), H.ptr(chol), H.ptr(prec),
                   H.ptr(logdet), H.ptr(resp), H.ptr(ws), N, D, C, Rs, diag, reg_covar, tol, it0,
                   min(sync_every, max_iter - it0 + 1), max_iter, H.stream())
            if bool(((state[:, 3] != 0) | (bad != 0).any(1)).all()):
                break
        logdens = torch.empty(Rs, N, **f64)
        labels = torch.empty(Rs, N, dtype=torch.int32, device=dev)
        H.call("mmvae_gmm_score", H.ptr(X), H.ptr(weights), H.ptr(means), H.ptr(prec), H.ptr(logdet), H.ptr(logdens),
               H.ptr(resp), H.ptr(labels), N, D, C, Rs, diag, H.stream())
        degenerate = (bad != 0).any(1)
        parts.append({"weights": weights, "means": means, "covariances": cov, "cholesky": chol, "precisions_cholesky": prec,
                      "log_det": logdet,
                      "lower_bound": torch.where(degenerate, torch.full_like(state[:, 0], -math.inf), state[:, 0]),
                      "n_iter": state[:, 1].to(torch.int32), "converged": (state[:, 2] != 0) & ~degenerate,
                      "degenerate": degenerate, "labels": labels, "resp": resp, "log_density": logdens})
    out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    bound = out["lower_bound"].cpu().numpy()
    if bool(out["degenerate"].all()):
        raise ValueError(f"{who}: every restart met a covariance without a Cholesky factor (a component of a single row or of "
                         f"equal rows); reg_covar = {reg_covar}: increase it, or ask for fewer components")
    out["best"] = int(np.argmax(bound))      # (degenerate restarts hold -inf; the first of equals)
    out["covariance_type"] = covariance_type
    return out


def _gmm_mixture(who, fit, restart):
    """one mixture out of what gmm_fit returns (`restart`, None: its best) or of a single mixture's entry (weights (C,), as
    TorchMMVAE.fit_latent_density returns per subset; `restart` must be None) or ValueError
    -> ({"weights" (C,), "means" (C,D), "cholesky", "precisions_cholesky", "log_det" (C,)}: contiguous float64, diag, restart)"""
    keys = ("weights", "means", "cholesky", "precisions_cholesky", "log_det")
    if not isinstance(fit, dict) or any(not torch.is_tensor(fit.get(k)) or fit[k].dtype != torch.float64 for k in keys) or \
            "covariance_type" not in fit:
        raise ValueError(f"{who}: fit is what gmm_fit returns (float64 {', '.join(keys)}; covariance_type)")
    diag = _gmm_covariance(who, fit["covariance_type"])
    many = fit["weights"].dim() == 2
    if many:
        R = fit["weights"].shape[0]
        restart = fit.get("best") if restart is None else restart
        if not isinstance(restart, (int, np.integer)) or not 0 <= restart < R:
            raise ValueError(f"{who}: restart = {restart!r} (the fit holds the restarts 0 .. {R - 1})")
        if "degenerate" in fit and bool(fit["degenerate"][restart]):
            raise ValueError(f"{who}: restart {restart} is degenerate (a covariance without a Cholesky factor)")
        restart = int(restart)
    elif restart is not None:
        raise ValueError(f"{who}: restart = {restart!r} for a single mixture (None)")
    m = {k: (fit[k][restart] if many else fit[k]).detach().contiguous() for k in keys}
    C = m["weights"].shape[0] if m["weights"].dim() == 1 else 0
    D = m["means"].shape[1] if m["means"].dim() == 2 else 0
    shape = (C, D) if diag else (C, D, D)
    if not 1 <= C <= H.CLUSTER_MAX_K or not 1 <= D <= H.GMM_MAX_D or m["means"].shape != (C, D) or m["log_det"].shape != (C,) or \
            m["cholesky"].shape != shape or m["precisions_cholesky"].shape != shape:
        raise ValueError(f"{who}: fit holds weights {tuple(m['weights'].shape)}, means {tuple(m['means'].shape)}, factors "
                         f"{tuple(m['cholesky'].shape)}; (C), (C, D) and {'(C, D)' if diag else '(C, D, D)'} with C <= "
                         f"{H.CLUSTER_MAX_K}, D <= {H.GMM_MAX_D} are on the MI355X path")
    return m, diag, restart


def gmm_score(X, fit, restart=None):
    """The log-density of the rows of X (N,D) under one mixture of `fit` (gmm_fit's result and a restart, None: its best; or a
    single mixture's entry), by the E-step's kernel: on the fitted rows it returns the fit's own bits.
    -> {"log_density" (N,) float64, "labels" (N,) int32 (the first most probable component), "resp" (N,C), "score": the mean}"""
    who = "gmm_score"
    m, diag, _ = _gmm_mixture(who, fit, restart)
    C, D = m["means"].shape
    X = _gmm_rows(who, X, D)
    N = X.shape[0]
    ck.need_gpu(who, "X is", X.device, "the kernels run")
    m = {k: v.to(X.device) for k, v in m.items()}
    logdens = torch.empty(N, dtype=torch.float64, device=X.device)
    resp = torch.empty(N, C, dtype=torch.float64, device=X.device)
    labels = torch.empty(N, dtype=torch.int32, device=X.device)
    H.call("mmvae_gmm_score", H.ptr(X), H.ptr(m["weights"]), H.ptr(m["means"]), H.ptr(m["precisions_cholesky"]),
           H.ptr(m["log_det"]), H.ptr(logdens), H.ptr(resp), H.ptr(labels), N, D, C, 1, diag, H.stream())
    return {"log_density": logdens, "labels": labels, "resp": resp, "score": float(logdens.cpu().numpy().mean())}


def gmm_sample(fit, n, u=None, eps=None, state=None, restart=None):
    """n draws from one mixture of `fit` (as in gmm_score): draw i takes the first component k with u[i] < w_0 + .. + w_k (the
    last one takes the rest) and z = mu_k + L_k eps[i] in double, rounded to fp32 once.  `u` (n,) float64 in [0, 1) (None:
    numpy.random.RandomState(0).random_sample(n)); `eps` (n,D) floats (None: ops.randn on `state`, the int32[3] state of the
    device generator).  -> (z (n,D) fp32, components (n,) int32)"""
    who = "gmm_sample"
    m, diag, _ = _gmm_mixture(who, fit, restart)
    C, D = m["means"].shape
    n = int(n)
    if not 1 <= n <= H.GMM_MAX_DRAWS:
        raise ValueError(f"{who}: n = {n} draws (1 .. {H.GMM_MAX_DRAWS} per call are on the MI355X path)")
    if u is None:
        u = torch.from_numpy(np.random.RandomState(0).random_sample(n))
    if isinstance(u, np.ndarray):
        u = torch.from_numpy(np.ascontiguousarray(u))
    if not torch.is_tensor(u) or u.dtype != torch.float64 or u.shape != (n,):
        raise ValueError(f"{who}: u is {ck.said(u)}; float64 ({n},) values in [0, 1)")
    if not bool(((u >= 0) & (u < 1)).all()):
        raise ValueError(f"{who}: u holds values outside [0, 1)")
    if eps is None:
        if not torch.is_tensor(state) or state.dtype != torch.int32 or state.numel() != 3:
            raise ValueError(f"{who}: without eps the draws need `state`, the int32[3] state of the device generator")
        from .. import ops      # (here, not at the top: ops imports this module; the generator's wrapper is the training path's)
        eps = ops.randn((n, D), state)
    if not torch.is_tensor(eps) or not eps.is_floating_point() or eps.shape != (n, D):
        raise ValueError(f"{who}: eps is {ck.said(eps)}; floating ({n}, {D}) standard-normal values")
    ck.finite(who, "eps", eps)
    dev = m["weights"].device
    ck.need_gpu(who, "the mixture is", dev, "the kernels run")
    u, eps = u.detach().to(dev).contiguous(), H.f32c(eps.detach().to(dev))
    z = torch.empty(n, D, dtype=torch.float32, device=dev)
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    H.call("mmvae_gmm_sample", H.ptr(m["weights"]), H.ptr(m["means"]), H.ptr(m["cholesky"]), H.ptr(u), H.ptr(eps), H.ptr(z),
           H.ptr(comp), n, D, C, diag, H.stream())
    return z, comp


def gmm_information(fit, n_rows, restart=None):
    """BIC and AIC of one mixture of `fit` on the n_rows rows it was fitted to, on the host, as scikit-learn's
    GaussianMixture.bic / .aic: n_parameters = C D (D + 1) / 2 + C D + C - 1 (full) or 2 C D + C - 1 (diag); with score = the
    mean log-density of those rows (`fit["log_density"]` of the restart, or a single mixture's `fit["score"]`):
    bic = -2 N score + n_parameters ln N, aic = -2 N score + 2 n_parameters.  -> {"n_parameters", "bic", "aic"}"""
    who = "gmm_information"
    if not isinstance(fit, dict) or not torch.is_tensor(fit.get("means")) or "covariance_type" not in fit:
        raise ValueError(f"{who}: fit is what gmm_fit returns (means, covariance_type, log_density)")
    diag = _gmm_covariance(who, fit["covariance_type"])
    n_rows = int(n_rows)
    if n_rows < 1:
        raise ValueError(f"{who}: n_rows = {n_rows}")
    C, D = fit["means"].shape[-2:]
    if fit["means"].dim() == 3:
        R = fit["means"].shape[0]
        restart = fit.get("best") if restart is None else restart
        if not isinstance(restart, (int, np.integer)) or not 0 <= restart < R:
            raise ValueError(f"{who}: restart = {restart!r} (the fit holds the restarts 0 .. {R - 1})")
        rows = fit["log_density"][restart]
        if rows.shape[0] != n_rows:
            raise ValueError(f"{who}: n_rows = {n_rows}, the fit holds the log-density of {rows.shape[0]} rows")
        score = float(rows.detach().cpu().numpy().mean())
    else:
        if restart is not None:
            raise ValueError(f"{who}: restart = {restart!r} for a single mixture (None)")
        score = float(fit["score"])
    n_par = (2 * C * D if diag else C * D * (D + 1) // 2 + C * D) + C - 1
    return {"n_parameters": n_par, "bic": -2.0 * score * n_rows + n_par * math.log(n_rows),
            "aic": -2.0 * score * n_rows + 2 * n_par}
