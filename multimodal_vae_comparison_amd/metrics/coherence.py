"""Generation coherence (csrc/coherence.hip): scoring kernels, forward only, no autograd."""
import ctypes

import torch

from .. import hipops as H

__all__ = ["text_decode_score", "cls_head"]


def text_decode_score(logits, target_ids=None, lengths=None):
    """logits (N,T,V) fp32 -> pred (N,T) int32: the first maximum over V of every step (an all-zero row gives 0).
    With target_ids (N,T) int32 and lengths (N,) int32 also letters (N,) int32: the steps t < min(lengths[n], T) at which
    pred equals the target (None without targets)."""
    assert logits.dim() == 3 and logits.dtype == torch.float32, "logits: fp32 (N,T,V)"
    logits = logits.contiguous()
    N, T, V = logits.shape
    if not (1 <= T <= H.COH_MAX_STEPS and 2 <= V <= H.COH_MAX_VOCAB):
        raise ValueError(f"text_decode_score: T = {T}, V = {V} (1 .. {H.COH_MAX_STEPS} steps, 2 .. {H.COH_MAX_VOCAB} "
                         f"symbols are on the MI355X path)")
    if (target_ids is None) != (lengths is None):
        raise ValueError("text_decode_score: target_ids and lengths come together")
    pred = torch.empty(N, T, dtype=torch.int32, device=logits.device)
    letters = None
    if N == 0:
        return pred, (None if target_ids is None else torch.empty(0, dtype=torch.int32, device=logits.device))
    if target_ids is not None:
        assert target_ids.shape == (N, T) and target_ids.dtype == torch.int32 and target_ids.is_contiguous()
        assert lengths.shape == (N,) and lengths.dtype == torch.int32 and lengths.is_contiguous()
        letters = torch.empty(N, dtype=torch.int32, device=logits.device)
    H.call("mmvae_text_decode_score", H.ptr(logits), H.ptr(target_ids), H.ptr(lengths), H.ptr(pred), H.ptr(letters), N, T,
           V, H.stream())
    return pred, letters


def cls_head(feats, W1, b1, W2, b2, n_classes, labels=None, want_logits=False):
    """The heads of A attribute classifiers in one launch.  feats (A,N,512): the trunks' last conv output before its
    ReLU; W1 (A,256,512), b1 (A,256), W2 (A,Cmax,256), b2 (A,Cmax); n_classes: A ints; labels (A,N) int32 or None
    (-1: never correct).  -> {"pred" (A,N) int32, "logits" (A,N,Cmax) or None, "correct" (A,N) uint8 and "n_correct"
    (N,) int32 (None without labels)}."""
    assert feats.dim() == 3 and feats.dtype == torch.float32 and feats.is_contiguous(), "feats: contiguous fp32 (A,N,512)"
    A, N, F_ = feats.shape
    n_classes = [int(c) for c in n_classes]
    Cmax = W2.shape[1]
    if not 1 <= A <= H.COH_MAX_CLASSIFIERS or len(n_classes) != A:
        raise ValueError(f"cls_head: {A} classifiers, {len(n_classes)} class counts (1 .. {H.COH_MAX_CLASSIFIERS} per "
                         f"launch)")
    if not 2 <= Cmax <= H.COH_MAX_CLASSES or any(not 2 <= c <= Cmax for c in n_classes):
        raise ValueError(f"cls_head: class counts {n_classes} under Cmax = {Cmax} (2 .. {H.COH_MAX_CLASSES} are on the "
                         f"MI355X path)")
    assert F_ == H.COH_FEATS and W1.shape == (A, H.COH_HIDDEN, H.COH_FEATS) and b1.shape == (A, H.COH_HIDDEN)
    assert W2.shape == (A, Cmax, H.COH_HIDDEN) and b2.shape == (A, Cmax)
    for t in (W1, b1, W2, b2):
        assert t.dtype == torch.float32 and t.is_contiguous(), "cls_head: contiguous fp32 parameters"
    dev = feats.device
    pred = torch.empty(A, N, dtype=torch.int32, device=dev)
    logits = torch.empty(A, N, Cmax, device=dev) if want_logits else None
    correct = n_correct = None
    if labels is not None:
        assert labels.shape == (A, N) and labels.dtype == torch.int32 and labels.is_contiguous(), "labels: int32 (A,N)"
        correct = torch.empty(A, N, dtype=torch.uint8, device=dev)
        n_correct = torch.empty(N, dtype=torch.int32, device=dev)
    if N > 0:
        H.call("mmvae_cls_head", H.ptr(feats), H.ptr(W1), H.ptr(b1), H.ptr(W2), H.ptr(b2), (ctypes.c_int * A)(*n_classes),
               H.ptr(labels), H.ptr(pred), H.ptr(logits), H.ptr(correct), H.ptr(n_correct), A, N, Cmax, H.stream())
    return {"pred": pred, "logits": logits, "correct": correct, "n_correct": n_correct}
