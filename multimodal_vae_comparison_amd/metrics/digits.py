"""MNIST-SVHN digit classifiers (csrc/digits.hip): evaluated and trained on chip, no autograd."""
import ctypes

import torch

from .. import hipops as H
from .probe import _check_order

__all__ = ["DIGIT_KINDS", "DIGIT_INPUT", "DIGIT_N_PARAMS", "digit_param_shapes", "digit_default_init", "digit_pack",
           "digit_unpack", "digit_state", "digit_check_labels", "digit_eval", "digit_grad", "digit_train", "digit_masks",
           "digit_hidden"]


DIGIT_KINDS = {"mnist": H.DIGIT_MNIST, "svhn": H.DIGIT_SVHN}
DIGIT_INPUT = {"mnist": (1, 28, 28), "svhn": (3, 32, 32)}
DIGIT_N_PARAMS = {"mnist": 21840, "svhn": 31340}


def digit_param_shapes(kind):
    """[(state-dict key, shape)] of a digit classifier in the packed order of the C ABI (the reference's module names)"""
    C, flat = DIGIT_INPUT[kind][0], (320 if kind == "mnist" else 500)
    return [("conv1.weight", (10, C, 5, 5)), ("conv1.bias", (10,)), ("conv2.weight", (20, 10, 5, 5)), ("conv2.bias", (20,)),
            ("fc1.weight", (50, flat)), ("fc1.bias", (50,)), ("fc2.weight", (10, 50)), ("fc2.bias", (10,))]


def _digit_kinds(kinds):
    kinds = [kinds] if isinstance(kinds, str) else list(kinds)
    if not 1 <= len(kinds) <= H.DIGIT_MAX_NETS or any(k not in DIGIT_KINDS for k in kinds):
        raise ValueError(f"digit classifiers: kinds = {kinds} (1 .. {H.DIGIT_MAX_NETS} of 'mnist' / 'svhn')")
    return kinds


def digit_default_init(kind, generator):
    """nn.Conv2d's / nn.Linear's default init -- weight and bias ~ U(-1/sqrt(fan_in), 1/sqrt(fan_in)) -- drawn on the
    host from `generator`, in the packed order -> {key: tensor}"""
    out = {}
    shapes = digit_param_shapes(kind)
    for (kw, sw), (kb, sb) in zip(shapes[0::2], shapes[1::2]):
        fan_in = 1
        for s in sw[1:]:
            fan_in *= s
        bound = 1.0 / fan_in ** 0.5
        out[kw] = (torch.rand(*sw, generator=generator) * 2.0 - 1.0) * bound
        out[kb] = (torch.rand(*sb, generator=generator) * 2.0 - 1.0) * bound
    return out


def digit_pack(kind, params):
    """{key: tensor} -> the packed (n_params,) fp32 host vector"""
    parts = []
    for k, s in digit_param_shapes(kind):
        t = params[k].detach().float().cpu()
        assert tuple(t.shape) == s, (k, tuple(t.shape), s)
        parts.append(t.reshape(-1))
    return torch.cat(parts)


def digit_unpack(kind, vec):
    """a packed (>= n_params,) vector -> {key: tensor} (copies, on vec's device)"""
    out, o = {}, 0
    for k, s in digit_param_shapes(kind):
        n = 1
        for d in s:
            n *= d
        out[k] = vec[o:o + n].reshape(s).clone()
        o += n
    return out


def digit_state(kinds, device, init=None, seed=0):
    """(nets, 3, n_params_max) fp32: [parameters | exp_avg | exp_avg_sq] per network in the packed order conv1.w, conv1.b,
    conv2.w, conv2.b, fc1.w, fc1.b, fc2.w, fc2.b.  The init is nn.Conv2d's / nn.Linear's default, drawn on the host from
    torch.Generator(seed) network after network, or `init`: one {state-dict key: tensor} per network.  Moments start at 0."""
    kinds = _digit_kinds(kinds)
    stride = max(DIGIT_N_PARAMS[k] for k in kinds)
    state = torch.zeros(len(kinds), 3, stride)
    g = torch.Generator().manual_seed(int(seed))
    if init is not None:
        assert len(init) == len(kinds), "init: one parameter dict per network"
    for i, k in enumerate(kinds):
        par = digit_default_init(k, g) if init is None else init[i]
        state[i, 0, :DIGIT_N_PARAMS[k]] = digit_pack(k, par)
    return state.to(device)


def _digit_args(state, kinds, images, labels=None):
    """shape contract of the digit entry points -> (kinds, host kind table, image pointer table, label pointer table, N)"""
    kinds = _digit_kinds(kinds)
    nets = len(kinds)
    assert state.dim() == 3 and state.shape[:2] == (nets, 3) and state.dtype == torch.float32 and state.is_contiguous(), \
        "state: contiguous fp32 (nets, 3, n_params_max)"
    assert state.shape[2] >= max(DIGIT_N_PARAMS[k] for k in kinds), "state: narrower than the largest network"
    assert len(images) == nets, "images: one (N,C,H,W) tensor per network"
    N = images[0].shape[0]
    for k, x in zip(kinds, images):
        assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (N,) + DIGIT_INPUT[k], \
            f"{k} images: contiguous fp32 (N,{','.join(map(str, DIGIT_INPUT[k]))}), got {tuple(x.shape)}"
    lab = None
    if labels is not None:
        assert len(labels) == nets, "labels: one (N,) int32 tensor per network"
        for y in labels:
            assert y.dtype == torch.int32 and y.is_contiguous() and tuple(y.shape) == (N,), "labels: contiguous int32 (N,)"
        lab = (H.c_p * nets)(*[H.ptr(y) for y in labels])
    return kinds, (ctypes.c_int * nets)(*[DIGIT_KINDS[k] for k in kinds]), (H.c_p * nets)(*[H.ptr(x) for x in images]), lab, N


def digit_check_labels(labels):
    """ValueError if a label lies outside [0, 10) (one host synchronisation per tensor)"""
    for y in labels:
        lo, hi = int(y.min()), int(y.max())
        if lo < 0 or hi >= 10:
            raise ValueError(f"digit classifiers: labels in [{lo}, {hi}], outside [0, 10)")


def _digit_p(p):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"digit classifiers: dropout p = {p} (0 <= p < 1)")
    return p


def digit_eval(state, kinds, images):
    """-> (logp (nets,N,10) fp32 log-probabilities, pred (nets,N) int32: their first maximum); dropout off"""
    kinds, ktab, xtab, _, N = _digit_args(state, kinds, images)
    dev = state.device
    logp = torch.empty(len(kinds), N, 10, device=dev)
    pred = torch.empty(len(kinds), N, dtype=torch.int32, device=dev)
    if N > 0:
        H.call("mmvae_digit_eval", H.ptr(state), ktab, xtab, H.ptr(logp), H.ptr(pred), len(kinds), state.shape[2], N,
               H.stream())
    return logp, pred


def digit_grad(state, kinds, images, labels, seed=0, step=0, p=0.0, validate=True):
    """The first half of a training step on one minibatch (all N rows of `images`): -> (grad (nets, n_params_max): the
    gradient of the mean loss with the dropout masks of (seed, step), rowloss (nets,N) = -logp[label])"""
    kinds, ktab, xtab, ltab, N = _digit_args(state, kinds, images, labels)
    if not 1 <= N <= 65535:
        raise ValueError(f"digit_grad: a minibatch of {N} rows (1 .. 65535)")
    if validate:
        digit_check_labels(labels)
    nets, stride, dev = len(kinds), state.shape[2], state.device
    ws = H.workspace(H.lib().mmvae_digit_ws_floats(nets, N, stride), dev)
    grad = torch.zeros(nets, stride, device=dev)
    rowloss = torch.empty(nets, N, device=dev)
    H.call("mmvae_digit_grad", H.ptr(state), ktab, xtab, ltab, H.ptr(ws), H.ptr(grad), H.ptr(rowloss), nets, stride, N,
           int(seed) & 0xFFFFFFFF, int(step), _digit_p(p), H.stream())
    return grad, rowloss


def digit_train(state, kinds, images, labels, batch, step0, n_steps, lr=1e-3, seed=0, p=0.5, order=None, validate=True):
    """Adam steps [step0, step0 + n_steps) of every network, in place on `state`: forward with dropout, backward, Adam;
    two launches per step.  images: per network (N,C,H,W) fp32 on the device, labels: per network (N,) int32; the
    minibatch schedule and `order` (E,N) int32 are ops.probe_train's.  -> loss (nets, n_steps)."""
    kinds, ktab, xtab, ltab, N = _digit_args(state, kinds, images, labels)
    batch, step0, n_steps = int(batch), int(step0), int(n_steps)
    if not 1 <= batch <= 65535 or n_steps < 1 or step0 < 0 or N < 1:
        raise ValueError(f"digit_train: batch = {batch}, step0 = {step0}, n_steps = {n_steps}, N = {N}")
    E = _check_order("digit_train", order, N, batch, step0, n_steps, validate, lambda: digit_check_labels(labels))
    nets, stride, dev = len(kinds), state.shape[2], state.device
    ws = H.workspace(H.lib().mmvae_digit_ws_floats(nets, batch, stride), dev)
    loss = torch.empty(nets, n_steps, device=dev)
    H.call("mmvae_digit_train", H.ptr(state), ktab, xtab, ltab, H.ptr(order), E, H.ptr(ws), H.ptr(loss), nets, stride, N,
           batch, step0, n_steps, float(lr), int(seed) & 0xFFFFFFFF, _digit_p(p), H.stream())
    return loss


def digit_masks(kind, batch, step0, n_steps, seed=0, p=0.5, device="cuda"):
    """The masks digit_train / digit_grad use for the steps [step0, step0 + n_steps) of a network kind, as 0 or 1/(1-p)
    floats -> (Dropout2d mask (n_steps, batch, 20), dropout mask (n_steps, batch, 50))"""
    (kind,) = _digit_kinds(kind)
    batch, n_steps = int(batch), int(n_steps)
    if not 1 <= batch <= 65535 or n_steps < 1 or int(step0) < 0:
        raise ValueError(f"digit_masks: batch = {batch}, step0 = {step0}, n_steps = {n_steps}")
    m2d = torch.empty(n_steps, batch, 20, device=device)
    m1 = torch.empty(n_steps, batch, 50, device=device)
    H.call("mmvae_digit_masks", H.ptr(m2d), H.ptr(m1), DIGIT_KINDS[kind], int(seed) & 0xFFFFFFFF, int(step0), n_steps,
           batch, _digit_p(p), H.stream())
    return m2d, m1


def digit_hidden(state, kinds, images):
    """-> (nets,N,50) fp32: relu(fc1) of the digit classifiers, dropout off (the features of DigitClassifier.features)"""
    kinds, ktab, xtab, _, N = _digit_args(state, kinds, images)
    hidden = torch.empty(len(kinds), N, 50, device=state.device)
    if N > 0:
        H.call("mmvae_digit_hidden", H.ptr(state), ktab, xtab, H.ptr(hidden), len(kinds), state.shape[2], N, H.stream())
    return hidden
