"""Latent analysis (csrc/tsne.hip): exact t-SNE, forward only, no autograd."""
import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["TSNE_SWITCH_IT", "TSNE_CHECK_EVERY", "tsne_sqdist", "tsne_default_init", "tsne_check_perplexity",
           "tsne_joint_probabilities", "tsne_state", "tsne_forces", "tsne_default_lr", "tsne_run", "tsne_embed"]


TSNE_SWITCH_IT = 250      # iterations with early exaggeration 12 and momentum 0.5 (scikit-learn's _EXPLORATION_MAX_ITER)
TSNE_CHECK_EVERY = 50     # iterations per enqueued call and between two looks at the log (its _N_ITER_CHECK)


def _tsne_points(who, X):
    assert X.dim() == 2 and X.dtype == torch.float32, f"{who}: fp32 (N, D)"
    N, D = X.shape
    if not H.TSNE_MIN_POINTS <= N <= H.TSNE_MAX_POINTS or not 1 <= D <= H.TSNE_MAX_DIM:
        raise ValueError(f"{who}: N = {N} points of D = {D} dimensions ({H.TSNE_MIN_POINTS} .. {H.TSNE_MAX_POINTS} points "
                         f"of 1 .. {H.TSNE_MAX_DIM} dimensions are on the MI355X path)")
    return N, D


def tsne_sqdist(X):
    """X (N,D) fp32 -> D2 (N,N) fp32: the squared Euclidean distances, every one summed directly in double and rounded
    (no Gram trick: near-duplicates do not cancel); zero diagonal, symmetric bit for bit."""
    N, D = _tsne_points("tsne_sqdist", X)
    X = X.contiguous()
    D2 = torch.empty(N, N, device=X.device)
    H.call("mmvae_tsne_sqdist", H.ptr(X), H.ptr(D2), N, D, H.stream())
    return D2


def tsne_default_init(N, seed=123):
    """scikit-learn's init="random": 1e-4 * RandomState(seed).standard_normal((N, 2)) as float32 (a host tensor)"""
    return torch.from_numpy((1e-4 * np.random.RandomState(int(seed)).standard_normal((int(N), 2))).astype(np.float32))


def tsne_check_perplexity(perplexity, N):
    if not float(perplexity) > 0.0:
        raise ValueError(f"perplexity must be positive, got {perplexity}")
    if float(perplexity) >= N:
        raise ValueError("perplexity must be less than n_samples")


def tsne_joint_probabilities(X, perplexity, sqdist=None, details=False):
    """-> (P (N,N) fp32, beta (N,) float64): scikit-learn's _joint_probabilities of the squared distances of X (or of
    `sqdist` (N,N) fp32 as given) -- per row the binary search for the precision beta that gives the conditional
    distribution the entropy log(perplexity), in double; P = max((C + C^T) / sum, eps) off the diagonal, 0 on it,
    symmetric bit for bit.  P is a view of rows padded to a multiple of 4 columns, the layout the iteration kernels read.
    `details`: also {"s", "rowsum", "steps"} of the search, (N,) float64 each."""
    D2 = tsne_sqdist(X) if sqdist is None else sqdist.contiguous()
    assert D2.dim() == 2 and D2.shape[0] == D2.shape[1] and D2.dtype == torch.float32, "sqdist: fp32 (N,N)"
    N = D2.shape[0]
    if not H.TSNE_MIN_POINTS <= N <= H.TSNE_MAX_POINTS:
        raise ValueError(f"tsne_joint_probabilities: N = {N} points ({H.TSNE_MIN_POINTS} .. {H.TSNE_MAX_POINTS} are on the "
                         f"MI355X path)")
    tsne_check_perplexity(perplexity, N)
    ld = H.lib().mmvae_tsne_ld(N)
    store = torch.empty(N, ld, device=D2.device)
    info = torch.empty(N, 4, dtype=torch.float64, device=D2.device)
    total = torch.empty(1, dtype=torch.float64, device=D2.device)
    H.call("mmvae_tsne_joint_p", H.ptr(D2), float(perplexity), H.ptr(store), ld, H.ptr(info), H.ptr(total), N, H.stream())
    P = store[:, :N]
    if details:
        return P, info[:, 0].clone(), {"s": info[:, 1].clone(), "rowsum": info[:, 2].clone(), "steps": info[:, 3].clone()}
    return P, info[:, 0].clone()


def _tsne_padded(P):
    """P (N,N) fp32 as the kernels read it: unit column stride, a row stride of N rounded up to 4 (16-byte rows) -- the
    view tsne_joint_probabilities returns as it is, anything else copied into that layout"""
    assert P.dim() == 2 and P.shape[0] == P.shape[1] and P.dtype == torch.float32, "P: fp32 (N,N)"
    N = P.shape[0]
    ld = (N + 3) & ~3
    if P.stride(1) == 1 and P.stride(0) == ld and P.data_ptr() % 16 == 0:
        return P, ld
    store = torch.zeros(N, ld, device=P.device)
    store[:, :N] = P
    return store[:, :N], ld


def tsne_state(Y0):
    """Y0 (N,2) -> the iteration's state (3,N,2) fp32 on the device Y0 is on: Y | upd = 0 | gains = 1"""
    assert Y0.dim() == 2 and Y0.shape[1] == 2, "Y0: (N,2)"
    Y0 = Y0.detach().float()
    return torch.stack([Y0, torch.zeros_like(Y0), torch.ones_like(Y0)]).contiguous()


def _tsne_args(who, state, P):
    assert state.dim() == 3 and state.shape[0] == 3 and state.shape[2] == 2 and state.dtype == torch.float32 \
        and state.is_contiguous(), "state: contiguous fp32 (3,N,2) from tsne_state"
    N = state.shape[1]
    if not H.TSNE_MIN_POINTS <= N <= H.TSNE_MAX_POINTS:
        raise ValueError(f"{who}: N = {N} points ({H.TSNE_MIN_POINTS} .. {H.TSNE_MAX_POINTS} are on the MI355X path)")
    assert P.shape[0] == N, f"{who}: P is {tuple(P.shape)}, the state holds {N} points"
    P, ld = _tsne_padded(P)
    ws = torch.empty(H.lib().mmvae_tsne_ws_doubles(N), dtype=torch.float64, device=state.device)
    return N, P, ld, ws


def tsne_forces(state, P, it, switch_it=TSNE_SWITCH_IT):
    """The first half of iteration `it` (exaggeration 12 for it < switch_it, then 1), the state untouched
    -> (g (N,2) fp32: the gradient of the objective, KL, Z: 0-d float64 tensors on the device)."""
    N, P, ld, ws = _tsne_args("tsne_forces", state, P)
    g = torch.empty(N, 2, device=state.device)
    kz = torch.empty(2, dtype=torch.float64, device=state.device)
    H.call("mmvae_tsne_forces", H.ptr(state), H.ptr(P), ld, H.ptr(ws), H.ptr(g), H.ptr(kz), N, int(it), int(switch_it),
           H.stream())
    return g, kz[0], kz[1]


def tsne_default_lr(N):
    """scikit-learn's learning_rate="auto": max(N / early_exaggeration / 4, 50)"""
    return max(N / 12.0 / 4.0, 50.0)


def tsne_run(state, P, it0, n_iter, lr, switch_it=TSNE_SWITCH_IT, kl_every=1):
    """The iterations [it0, it0 + n_iter) in place on `state`, enqueued in one call (two launches per iteration, no host
    synchronisation) -> log (n_iter,2) float64 on the device: (KL with the iteration's exaggeration, |g|_2) at the
    embedding each iteration started from.  `kl_every`: KL is computed in the iterations with (it + 1) % kl_every == 0,
    NaN elsewhere (scikit-learn computes it every 50th; its double logarithms are most of a pair's arithmetic).
    Bit-identical from run to run and however the iterations are split over calls."""
    N, P, ld, ws = _tsne_args("tsne_run", state, P)
    if int(n_iter) < 1 or int(it0) < 0 or not float(lr) > 0.0 or int(kl_every) < 1:
        raise ValueError(f"tsne_run: it0 = {it0}, n_iter = {n_iter}, lr = {lr}, kl_every = {kl_every}")
    log = torch.empty(int(n_iter), 2, dtype=torch.float64, device=state.device)
    H.call("mmvae_tsne_run", H.ptr(state), H.ptr(P), ld, H.ptr(ws), H.ptr(log), N, int(it0), int(n_iter), int(switch_it),
           float(lr), int(kl_every), H.stream())
    return log


def tsne_embed(X, perplexity=30.0, max_iter=1000, seed=123, init=None, lr="auto", n_iter_without_progress=300,
               min_grad_norm=1e-7, kl_every=TSNE_CHECK_EVERY):
    """Exact t-SNE of X (N,D) fp32 into two dimensions: sklearn.manifold.TSNE(n_components=2, method="exact",
    init="random", random_state=seed, learning_rate="auto") -- 250 iterations with early exaggeration 12 and momentum 0.5,
    then momentum 0.8 up to `max_iter`, with scikit-learn's stopping rule: every 50th iteration a stage ends when the
    objective has had no new best for more than `n_iter_without_progress` iterations (250 in the first stage) or when
    |g|_2 <= min_grad_norm.  (scikit-learn takes the norm of the gradient scaled by the gains; here it is the gradient's.)
    `init`: (N,2) instead of the seeded draw.  The host enqueues 50 iterations per call and reads the log back once per
    call: at most max_iter / 50 synchronisations.
    -> {"embedding": (N,2) fp32, "kl_divergence": float, the objective at the returned embedding without exaggeration,
        "n_iter": iterations run, "log": (n_iter,2) float64 (KL, |g|) per iteration (KL every `kl_every`-th, NaN between),
        "beta": (N,) float64 precisions of the perplexity search}."""
    N, _ = _tsne_points("tsne_embed", X)
    tsne_check_perplexity(perplexity, N)
    max_iter = int(max_iter)
    if max_iter < TSNE_SWITCH_IT:
        raise ValueError(f"tsne_embed: max_iter = {max_iter} (at least the {TSNE_SWITCH_IT} iterations of the first stage)")
    if TSNE_CHECK_EVERY % int(kl_every) != 0:
        raise ValueError(f"tsne_embed: kl_every = {kl_every} must divide the check cadence {TSNE_CHECK_EVERY}")
    ck.finite("tsne_embed", "X", X)
    lr = tsne_default_lr(N) if isinstance(lr, str) else float(lr)
    P, beta = tsne_joint_probabilities(X, perplexity)
    Y0 = tsne_default_init(N, seed) if init is None else torch.as_tensor(init)
    if tuple(Y0.shape) != (N, 2):
        raise ValueError(f"tsne_embed: init is {tuple(Y0.shape)}, not ({N}, 2)")
    state = tsne_state(Y0.to(X.device))
    logs, it, switch_it = [], 0, TSNE_SWITCH_IT
    for stage_end, patience in ((TSNE_SWITCH_IT, TSNE_SWITCH_IT), (max_iter, int(n_iter_without_progress))):
        best, best_it, stop = float("inf"), it, False
        while it < stage_end and not stop:
            n = min(TSNE_CHECK_EVERY - it % TSNE_CHECK_EVERY, stage_end - it)
            log = tsne_run(state, P, it, n, lr, switch_it=switch_it, kl_every=kl_every)
            logs.append(log)
            it += n
            if it % TSNE_CHECK_EVERY == 0:
                kl, gnorm = log[-1].tolist()      # (the synchronisation of this call)
                if kl < best:
                    best, best_it = kl, it - 1
                elif it - 1 - best_it > patience:
                    stop = True
                if gnorm <= float(min_grad_norm):
                    stop = True
        switch_it = min(switch_it, it)
    _, kl, _ = tsne_forces(state, P, max(it, switch_it), switch_it=switch_it)
    return {"embedding": state[0].clone(), "kl_divergence": float(kl), "n_iter": it, "log": torch.cat(logs),
            "beta": beta}
