"""Latent classification (csrc/probe.hip): linear probes trained on chip, forward only, no autograd; and the host
helpers of the evaluation metrics: labels, and the minibatch `order` of probe_train / digit_train."""
import ctypes

import torch

from .. import hipops as H

__all__ = ["label_matrix", "epoch_orders", "probe_check_labels", "probe_state", "probe_weights", "probe_train", "probe_eval"]


def label_matrix(batches, what, who):
    """labels of an iterable of (batch, labels) -> (A, N) int64 on the host; `who` names the caller in the errors"""
    cols = []
    for _, y in batches:
        y = torch.as_tensor(y).detach().cpu()
        if y.is_floating_point() or y.dim() not in (1, 2):
            raise ValueError(f"{who}: {what} labels must be an integer (B,) or (B, A) array")
        cols.append(y.long().reshape(y.shape[0], -1))
    if not cols:
        raise ValueError(f"{who}: the {what} set is empty")
    return torch.cat(cols, 0).t().contiguous()


def epoch_orders(N, epochs, seed, device, shuffle=True):
    """the `order` argument of probe_train / digit_train: (epochs, N) int32 on `device`, one permutation of the N rows per
    epoch drawn from torch.Generator(seed); None -- sequential minibatches -- when not shuffling"""
    if not shuffle:
        return None
    g = torch.Generator().manual_seed(int(seed))
    return torch.stack([torch.randperm(N, generator=g) for _ in range(int(epochs))]).to(device=device, dtype=torch.int32)


def _check_order(who, order, N, batch, step0, n_steps, validate, check_labels):
    """`order` of probe_train / digit_train: (E,N) contiguous int32, E epochs enough for the steps [step0, step0 + n_steps);
    under `validate` the caller's `check_labels()`, then every entry a row in [0, N).  -> E (0: sequential, no `order`)"""
    E = 0
    if order is not None:
        assert order.dim() == 2 and order.dtype == torch.int32 and order.is_contiguous() and order.shape[1] == N
        E = order.shape[0]
        spe = (N + batch - 1) // batch
        if (step0 + n_steps - 1) // spe >= E:
            raise ValueError(f"{who}: steps up to {step0 + n_steps} need more than the {E} epochs of `order`")
    if validate:
        check_labels()
        if order is not None and (int(order.min()) < 0 or int(order.max()) >= N):
            raise ValueError(f"{who}: `order` holds rows outside [0, N)")
    return E


def _probe_table(probes, Cmax):
    """[(s, a, C)] -> the host (P,3) int table of the C ABI.  The class counts are checked here (ValueError names them);
    the kernels refuse the same shapes with MMVAE_ERR_UNSUPPORTED."""
    probes = [tuple(int(x) for x in pr) for pr in probes]
    if not probes or len(probes) > H.PROBE_MAX_PROBES:
        raise ValueError(f"probe table: {len(probes)} probes (1 .. {H.PROBE_MAX_PROBES} per launch)")
    for s, a, C in probes:
        if not 2 <= C <= min(Cmax, H.PROBE_MAX_CLASSES):
            raise ValueError(f"probe table: {C} classes (2 .. {min(Cmax, H.PROBE_MAX_CLASSES)} are on the MI355X path)")
    flat = [x for pr in probes for x in pr]
    return probes, (ctypes.c_int * len(flat))(*flat)


def _probe_dims(state, z, probes):
    """shape contract shared by probe_train / probe_eval -> (P, S, N, D, Cmax)"""
    assert z.dim() == 3 and z.dtype == torch.float32 and z.is_contiguous(), "z: contiguous fp32 (S,N,D)"
    S, N, D = z.shape
    if D > 256:
        raise ValueError(f"probe: D = {D} latent dimensions (up to 256 are on the MI355X path)")
    assert state.dim() == 4 and state.shape[1] == 3 and state.dtype == torch.float32 and state.is_contiguous()
    P, Cmax = state.shape[0], state.shape[2]
    assert state.shape[3] == D + 1 and P == len(probes), "state: (P, 3, Cmax, D + 1), one row per probe"
    return P, S, N, D, Cmax


def probe_check_labels(labels, probes):
    """ValueError if a probe's label row holds a label outside [0, C) (one host synchronisation)"""
    lo, hi = labels.amin(1).tolist(), labels.amax(1).tolist()
    for s, a, C in probes:
        if not 0 <= int(a) < labels.shape[0]:
            raise ValueError(f"probe table: label row {a} of {labels.shape[0]}")
        if lo[a] < 0 or hi[a] >= C:
            raise ValueError(f"probe labels: row {a} holds labels in [{lo[a]}, {hi[a]}], outside [0, {C})")


def probe_state(P, D, Cmax, device, init=None, seed=0):
    """(P, 3, Cmax, D + 1) fp32: [parameters | exp_avg | exp_avg_sq] per probe, each a (Cmax, D + 1) matrix [W | b].
    nn.Linear's default init -- W and b ~ U(-1/sqrt(D), 1/sqrt(D)) -- drawn on the host from torch.Generator(seed), or
    the (W (C,D), b (C,)) pairs of `init` (rows beyond C stay 0).  The moments start at 0."""
    P, D, Cmax = int(P), int(D), int(Cmax)
    if D < 1 or D > 256:
        raise ValueError(f"probe: D = {D} latent dimensions (1 .. 256 are on the MI355X path)")
    if not 2 <= Cmax <= H.PROBE_MAX_CLASSES:
        raise ValueError(f"probe: {Cmax} classes (2 .. {H.PROBE_MAX_CLASSES} are on the MI355X path)")
    par = torch.zeros(P, Cmax, D + 1)
    if init is None:
        bound = 1.0 / D ** 0.5
        g = torch.Generator().manual_seed(int(seed))
        par.copy_((torch.rand(P, Cmax, D + 1, generator=g) * 2.0 - 1.0) * bound)
    else:
        assert len(init) == P, "init: one (W, b) pair per probe"
        for p, (W, b) in enumerate(init):
            C = W.shape[0]
            assert W.shape == (C, D) and b.shape == (C,) and C <= Cmax, (tuple(W.shape), tuple(b.shape), Cmax, D)
            par[p, :C, :D] = W.detach().float().cpu()
            par[p, :C, D] = b.detach().float().cpu()
    state = torch.zeros(P, 3, Cmax, D + 1)
    state[:, 0] = par
    return state.to(device)


def probe_weights(state, p, C):
    """-> (W (C,D), b (C,)) of probe p (copies)"""
    par = state[p, 0, :C]
    return par[:, :-1].clone(), par[:, -1].clone()


def probe_train(state, z, labels, probes, batch, step0, n_steps, lr=1e-3, order=None, validate=True):
    """Adam steps [step0, step0 + n_steps) of every probe in ONE launch (one workgroup per probe), in place on `state`.
    z (S,N,D) fp32, labels (A,N) int32, probes [(s, a, C)]; step t covers positions [i batch, (i + 1) batch) of epoch
    t // ceil(N / batch); `order` (E,N) int32 maps position -> row per epoch (None: sequential).
    -> loss (P, n_steps): the mean cross-entropy of every step.  `validate`: check labels / order on the host first."""
    P, S, N, D, Cmax = _probe_dims(state, z, probes)
    probes, table = _probe_table(probes, Cmax)
    assert labels.dim() == 2 and labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape[1] == N
    if int(batch) < 1 or int(n_steps) < 1 or int(step0) < 0:
        raise ValueError(f"probe_train: batch = {batch}, step0 = {step0}, n_steps = {n_steps}")
    E = _check_order("probe_train", order, N, int(batch), int(step0), int(n_steps), validate,
                     lambda: probe_check_labels(labels, probes))
    for s, a, C in probes:
        if not (0 <= s < S and 0 <= a < labels.shape[0]):
            raise ValueError(f"probe table: probe ({s}, {a}, {C}) outside {S} latent matrices / {labels.shape[0]} label rows")
    loss = torch.empty(P, int(n_steps), device=z.device)
    H.call("mmvae_probe_train", H.ptr(state), H.ptr(z), H.ptr(labels), H.ptr(order), E, table, H.ptr(loss), P, S,
           labels.shape[0], N, D, Cmax, int(batch), int(step0), int(n_steps), float(lr), H.stream())
    return loss


def probe_eval(state, z, labels, probes):
    """-> (pred (P,N) int32: argmax of the logits, the first maximum; nll (P,N) fp32: the row's cross-entropy against its
    probe's label row, 0 when `labels` is None)"""
    P, S, N, D, Cmax = _probe_dims(state, z, probes)
    probes, table = _probe_table(probes, Cmax)
    A = 0
    if labels is not None:
        assert labels.dim() == 2 and labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape[1] == N
        A = labels.shape[0]
    for s, a, C in probes:
        if not (0 <= s < S and (labels is None or 0 <= a < A)):
            raise ValueError(f"probe table: probe ({s}, {a}, {C}) outside {S} latent matrices / {A} label rows")
    pred = torch.empty(P, N, dtype=torch.int32, device=z.device)
    nll = torch.empty(P, N, device=z.device)
    H.call("mmvae_probe_eval", H.ptr(state), H.ptr(z), H.ptr(labels), table, H.ptr(pred), H.ptr(nll), P, S, A, N, D, Cmax,
           H.stream())
    return pred, nll
