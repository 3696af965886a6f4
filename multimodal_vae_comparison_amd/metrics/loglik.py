"""Held-out log-likelihood estimation (csrc/loglik.hip): forward only, no autograd."""
import ctypes

import torch

from .. import hipops as H

__all__ = ["mix_ksample_logw", "lme_state", "lme_update", "lme_finish"]


def mix_ksample_logw(comps, laplace, theta, Kc, k0=0, eps=None, rng=None, advance=True, prior_loc=None,
                     prior_laplace=False):
    """Stratified draws from the mixture q = (1/C) sum_c q_c and the latent part of their importance weights.
    comps (C,B,2D) = [loc | scale], laplace: C flags, theta (1,D): the prior's scale is softmax(theta) D.
    Draw k0 + k (k < Kc) comes from component (k0 + k) % C; its noise is eps[k] (eps (Kc,B,D)) or, with `rng` (the
    generator state), element (k0 + k) B D + b D + d of the current draw -- `advance` bumps the state's call counter and
    belongs to the last chunk of a draw.  -> z (Kc,B,D), lw0 (Kc,B) = log p(z) - log q(z)."""
    comps = H.f32c(comps)
    C, B, D2 = comps.shape
    D = D2 // 2
    assert len(laplace) == C and (eps is None) != (rng is None), "either eps or the generator state"
    if eps is not None:
        eps = H.f32c(eps)
        assert tuple(eps.shape) == (Kc, B, D), (tuple(eps.shape), (Kc, B, D))
    if prior_loc is not None:
        prior_loc = H.f32c(prior_loc)
        assert prior_loc.numel() == D
    theta = H.f32c(theta)
    assert theta.numel() == D
    z = torch.empty(Kc, B, D, device=comps.device)
    lw0 = torch.empty(Kc, B, device=comps.device)
    mask = sum(1 << c for c, f in enumerate(laplace) if f)
    H.call("mmvae_mix_ksample_logw_fwd", H.ptr(comps), mask, H.ptr(theta), H.ptr(prior_loc), int(bool(prior_laplace)),
           H.ptr(eps), H.ptr(rng), int(bool(advance)), H.ptr(z), H.ptr(lw0), C, int(Kc), int(k0), B, D, H.stream())
    return z, lw0


def lme_state(n_rows, B, device):
    """empty streaming log-sum-exp state (1 + n_rows, 3, B) fp64: running maximum -inf, both sums 0"""
    st = torch.zeros(1 + n_rows, 3, B, dtype=torch.float64, device=device)
    st[:, 0] = float("-inf")
    return st


def lme_update(state, lw0, rows, joint_mask=None):
    """fold one chunk into the state: row 0 takes lw0 + sum of the rows in `joint_mask` (default: all), row 1 + m takes
    rows[m].  lw0 and every row: (Kc,B) fp32."""
    lw0 = H.f32c(lw0)
    Kc, B = lw0.shape
    rows = [H.f32c(r).reshape(-1) for r in rows]
    assert state.dtype == torch.float64 and tuple(state.shape) == (1 + len(rows), 3, B) and state.is_contiguous()
    assert all(r.numel() == Kc * B for r in rows)
    t = H.LmeRows()
    for m, r in enumerate(rows):
        t.ll[m] = r.data_ptr()
    mask = (1 << len(rows)) - 1 if joint_mask is None else int(joint_mask)
    H.call("mmvae_lme_update", H.ptr(state), H.ptr(lw0), ctypes.byref(t), len(rows), mask, Kc, B, H.stream())
    return state


def lme_finish(state, K):
    """-> (log-mean-exp over the K folded samples (1 + n_rows, B), effective sample size of row 0 (B,)), fp64"""
    R, _, B = state.shape
    out = torch.empty(R, B, dtype=torch.float64, device=state.device)
    ess = torch.empty(B, dtype=torch.float64, device=state.device)
    H.call("mmvae_lme_finish", H.ptr(state), H.ptr(out), H.ptr(ess), R - 1, int(K), B, H.stream())
    return out, ess
