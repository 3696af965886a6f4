"""What counts as a valid operand of a metric kernel: the argument checks every metric module shares.

Every function takes `who` (the public function that was called) and `what` (the operand's name) and raises ValueError
before any C call; the limits and the clause that explains them are the caller's.  Nothing here knows a family: a
condition that only one kernel has (k + 1 rows for the k-th neighbour, restarts, perplexity, window sizes) stays in that
kernel's module.  A device read (a host synchronisation) happens in `finite` and `extremes` only, once per call."""
import numpy as np
import torch

from .. import hipops as H


def said(X):
    """how a wrong operand is described: shape and dtype of a tensor, otherwise the name of its type"""
    return f"{tuple(X.shape)}, {X.dtype}" if torch.is_tensor(X) else type(X).__name__


def _limits(who, shape, limits):
    """`limits`: (dimension, least, most, text) in the order of refusal; most None: unbounded; text: the refusal after
    "who: ", a format of the sizes ({0} the first dimension, ...; {shape} all of them)"""
    for dim, least, most, text in limits:
        if shape[dim] < least or (most is not None and shape[dim] > most):
            raise ValueError(f"{who}: " + text.format(*shape, shape=tuple(shape)))


def finite(who, what, X):
    if not bool(torch.isfinite(X).all()):
        raise ValueError(f"{who}: {what} holds values that are not finite")


def chunks(who, chunks, what="column chunks"):
    chunks = int(chunks)
    if chunks < 0:
        raise ValueError(f"{who}: chunks = {chunks} (0: the default plan, or a positive number of {what})")
    return chunks


def need_gpu(who, what_is, device, runs="the kernel runs"):
    """the refusal of a host tensor (`what_is`: "X is", "the moments are")"""
    if device.type != "cuda":
        raise ValueError(f"{who}: {what_is} on {device}; {runs} on the MI355X (there is no host path)")


def same_device(who, a_is, a, b, B):
    """two operands on different devices: `a_is` ("rad2 is") on a.device, `b` ("the manifold rows") on B.device"""
    if a.device != B.device:
        raise ValueError(f"{who}: {a_is} on {a.device}, {b} on {B.device}")


def same_features(who, a_has, a, b, B):
    """two (rows, F) operands of different F: `a_has` ("real has", "queries have"), `b` the other's name"""
    if a.shape[1] != B.shape[1]:
        raise ValueError(f"{who}: {a_has} F = {a.shape[1]} features, {b} F = {B.shape[1]}")


def floating(who, what, X, dims, form):
    """a floating tensor of `dims` dimensions or ValueError; `form`: what is wanted, after "floating" """
    if not torch.is_tensor(X) or X.dim() != dims or not X.is_floating_point():
        raise ValueError(f"{who}: {what} is {said(X)}; floating {form}")


def rows(who, what, X, dims, form, limits=(), like=None, strict=False, defer=False):
    """contiguous fp32 of `dims` dimensions, detached, or ValueError, in this order: a floating tensor of that rank
    (`floating`), the sizes inside `limits` (`_limits`), the shape and device of `like` = (its name, the tensor), contiguous
    as given (`strict`; otherwise it is made so), finite values (`defer`: the caller checks them, with `finite`, after
    comparisons of its own)"""
    floating(who, what, X, dims, form)
    _limits(who, X.shape, limits)
    if like is not None and (X.shape != like[1].shape or X.device != like[1].device):
        raise ValueError(f"{who}: {what} is {tuple(X.shape)} on {X.device}, {like[0]} {tuple(like[1].shape)} on "
                         f"{like[1].device}")
    if strict and not X.is_contiguous():
        raise ValueError(f"{who}: {what} is not contiguous")
    X = H.f32c(X.detach())
    if not defer:
        finite(who, what, X)
    return X


def feature_rows(who, what, X, least=1, most=None, why="", defer=False):
    """`rows` for (rows, F) features: the limit on F, then `least` .. `most` rows (`why`: the caller's clause on that limit)"""
    return rows(who, what, X, 2, "(rows, F) features",
                ((1, 1, H.FRECHET_MAX_F, f"{what} has F = {{1}} features (1 .. {H.FRECHET_MAX_F} are on the MI355X path)"),
                 (0, least, most, f"{what} has {{0}} rows ({why})")), defer=defer)


def extremes(t):
    """(smallest, largest) entry of an integer tensor: the ONE read of it that a call's validation makes"""
    return tuple(int(v) for v in torch.aminmax(t))


def integers(who, what, t, dims, form, limits=(), device=None, beside="", arrays=(), nonempty=False, strict=False,
             inside=None, to=torch.int32):
    """an integer tensor (not floating, complex or bool) or ValueError, in this order: a host array of the types `arrays`
    becomes a tensor; `dims` dimensions (None: any) -- `form` says what is wanted; the sizes inside `limits`; on `device`,
    where one is given (`beside`: what else is there); contiguous as given (`strict`); every entry inside [lo, hi) for
    `inside` = (lo, hi, text; a bound None: open; text: a format of the smallest and largest entry found).
    -> contiguous int32 (`to`), the tensor on the host (to="host") or as it is (to=None), detached"""
    if isinstance(t, arrays):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not torch.is_tensor(t) or (dims is not None and t.dim() != dims) or (nonempty and t.numel() == 0) or \
            t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{who}: {what} is {said(t)}; {form}")
    _limits(who, t.shape, limits)
    if device is not None and t.device != device:
        raise ValueError(f"{who}: {what} is on {t.device}, {beside} on {device}")
    if strict and not t.is_contiguous():
        raise ValueError(f"{who}: {what} is not contiguous")
    t = t.detach()
    if inside is not None and t.numel():
        lo, hi, text = inside
        least, most = extremes(t)
        if (lo is not None and least < lo) or (hi is not None and most >= hi):
            raise ValueError(f"{who}: {what} " + text.format(least, most))
    if to is None:
        return t
    return t.cpu() if to == "host" else t.to(to).contiguous()


def feature_count(who, F):
    F = int(F)
    if not 1 <= F <= H.FRECHET_MAX_F:
        raise ValueError(f"{who}: F = {F} features (1 .. {H.FRECHET_MAX_F} are on the MI355X path)")
    return F


def f64_square(who, what, M):
    """a contiguous float64 (F,F) matrix inside the limit on F, or ValueError"""
    if not torch.is_tensor(M) or M.dim() != 2 or M.shape[0] != M.shape[1] or M.dtype != torch.float64:
        raise ValueError(f"{who}: {what} of shape {said(M)}; float64 (F,F), 1 <= F <= {H.FRECHET_MAX_F} on the MI355X path")
    feature_count(who, M.shape[0])
    return M.contiguous()


def f64_block(who, what, M):
    """a float64 (rows, cols) tensor or view whose rows are contiguous (a sub-block of a row-major matrix), or ValueError"""
    if not torch.is_tensor(M) or M.dim() != 2 or M.dtype != torch.float64 or M.stride(1) != 1 or \
            M.stride(0) < M.shape[1] or not all(1 <= n <= H.FRECHET_MAX_F for n in M.shape):
        strides = f", strides {M.stride()}" if torch.is_tensor(M) else ""
        raise ValueError(f"{who}: {what} is {said(M)}{strides}; a float64 block (rows, cols) with contiguous rows, 1 .. "
                         f"{H.FRECHET_MAX_F} each way on the MI355X path")
    return M
