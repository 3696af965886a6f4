"""What tests/test_loss_gpu.py measures csrc/loss.hip against: float64 restatements of every loss kernel in plain torch
(no custom Functions; gradients in closed form), and the deterministic inputs of every case.  tests/
test_loss_reference_host.py pins the restatements to torch's own operations and autograd on the CPU, and asserts
that the inputs hold the edge values the GPU tests rely on (active clamps, exact targets, padded steps, ties, NaNs).

Conventions: a target with fewer rows than the output repeats (output row b against target row b % rows,
BaseObjective.reshape_for_loss, objectives.py:118-120).  lprob elements follow the dtype of their inputs -- float32
inputs give the reference's float32 element arithmetic followed by a cast to double (ReconLoss.lprob,
objectives.py:409-424; the convention of test_boundary_gpu._torch_reference), float64 inputs give float64."""
import functools
import math

import torch
import torch.distributions as dist
import torch.nn.functional as F

F64 = torch.float64
# the two float32 values clamp(sigmoid(.), 1e-6, 1 - 1e-6) can stop at; 1 - 1e-6 itself is no float32 value
ETA_LO = torch.tensor(1e-6, dtype=torch.float32)
ETA_HI = torch.tensor(1.0 - 1e-6, dtype=torch.float32)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
CAP = 2048 * 256          # elements the element-wise kernels cover before their grid-stride loop turns


def repeat_rows(target, B):
    """(rows, ...) -> (B, ...): the K-sample repeat the kernels never materialise"""
    return target.repeat(B // target.shape[0], *([1] * (target.dim() - 1)))


# ---------------------------------------------------------------------------------------------
# bce (ReconLoss.bce, objectives.py:392-406) on x_hat = clamp(sigmoid(logits), 1e-6, 1 - 1e-6)
# ---------------------------------------------------------------------------------------------
def bce_elems(x_hat, target):
    """F.binary_cross_entropy(reduction="none"): both logs clamped at -100"""
    x, t = x_hat.double(), target.double()
    return -(t * torch.log(x).clamp_min(-100.0) + (1.0 - t) * torch.log(1.0 - x).clamp_min(-100.0))


def bce_rows(x_hat, target):
    B = x_hat.shape[0]
    return bce_elems(x_hat.reshape(B, -1), repeat_rows(target.reshape(target.shape[0], -1), B)).sum(-1)


def bce_dxhat(x_hat, target, g_row):
    """d rows / d x_hat as torch computes it: g (x - t) / max((1 - x) x, 1e-12)"""
    x, t = x_hat.double(), target.double()
    return g_row.double()[:, None] * (x - t) / ((1.0 - x) * x).clamp_min(1e-12)


def clamp_active(x_hat):
    """decided from the INPUT: x_hat sits on one of the two clamp constants (float32 constants for float32 input)"""
    return (x_hat == ETA_LO.to(x_hat.dtype)) | (x_hat == ETA_HI.to(x_hat.dtype))


def bce_dlogit(x_hat, target, g_row):
    """d rows / d logits for x_hat = clamp(sigmoid(logits)): g (x_hat - t), exactly 0 where the clamp is active"""
    B = x_hat.shape[0]
    x, t = x_hat.double(), repeat_rows(target, B).double()
    return torch.where(clamp_active(x_hat), torch.zeros_like(x), g_row.double()[:, None] * (x - t))


def sigmoid_clamp_dlogit(y, dy):
    """backward of y = clamp(sigmoid(logits)) alone: dy y (1 - y), exactly 0 where the clamp is active"""
    v = y.double()
    return torch.where(clamp_active(y), torch.zeros_like(v), dy.double() * v * (1.0 - v))


# ---------------------------------------------------------------------------------------------
# category_ce with the softmax over TIME (objectives.py:486-500): logits (B,T,V), target (rows,T,V) -> (B,V)
# ---------------------------------------------------------------------------------------------
def ce_loss(logits, target):
    l, t = logits.double(), repeat_rows(target, logits.shape[0]).double()
    return -(t * F.log_softmax(l, dim=1)).sum(1)


def ce_dlogits(logits, target, g):
    """g: (B,V) upstream of the per-column loss, or (B,) upstream of its row sums"""
    l, t = logits.double(), repeat_rows(target, logits.shape[0]).double()
    gv = g.double()[:, None, :] if g.dim() == 2 else g.double()[:, None, None]
    return gv * (F.softmax(l, dim=1) * t.sum(1, keepdim=True) - t)


# ---------------------------------------------------------------------------------------------
# lprob (objectives.py:409-424): -log p(target) under Normal / Laplace(loc, scale), NaN -> 0 with no gradient;
# scale None = the masked-modality quirk scale := loc
# ---------------------------------------------------------------------------------------------
def row_is_laplace(B, laplace):
    """laplace: bool, or (bit mask, block rows): rows [j, j + 1) * block rows are Laplace where bit j is set"""
    if isinstance(laplace, tuple):
        return torch.tensor([bool((laplace[0] >> (b // laplace[1])) & 1) for b in range(B)])
    return torch.full((B,), bool(laplace))


def lprob_elems(loc, target, scale, laplace):
    """element arithmetic in the dtype of `loc` (torch.distributions' own expressions), then double, NaN -> 0"""
    s = loc if scale is None else torch.full_like(loc, float(scale))
    d = (dist.Laplace if laplace else dist.Normal)(loc, s, validate_args=False)
    lp = d.log_prob(target.to(loc.dtype)).double()
    return torch.where(torch.isnan(lp), torch.zeros_like(lp), -lp)


def lprob_velems(loc, target, scale, laplace):
    """d(-log p) / d loc per element in float64 from the given inputs; 0 where the element (in the inputs' dtype) or
    its derivative is NaN"""
    s_in = loc if scale is None else torch.full_like(loc, float(scale))
    lp = (dist.Laplace if laplace else dist.Normal)(loc, s_in, validate_args=False).log_prob(target.to(loc.dtype))
    x, t, s = loc.double(), target.double(), s_in.double()
    d = t - x
    if laplace:
        v = -torch.sign(d) / s
        if scale is None:
            v = v + 1.0 / s - d.abs() / (s * s)
    else:
        v = -d / (s * s)
        if scale is None:
            v = v + 1.0 / s - d * d / (s * s * s)
    return torch.where(torch.isnan(lp) | torch.isnan(v), torch.zeros_like(v), v)


def _paired(loc, target, perm_c):
    """loc (B, ...) and target (rows, ...) as (B, F) pairs; perm_c: loc is (B, perm_c, F / perm_c) in memory and meets
    the target as if permuted to (B, F / perm_c, perm_c) (Dec_SVHN)"""
    B = loc.shape[0]
    x = loc.reshape(B, -1)
    F_ = x.shape[1]
    if perm_c:
        x = x.reshape(B, perm_c, F_ // perm_c).transpose(1, 2).reshape(B, F_)
    return x, repeat_rows(target.reshape(target.shape[0], -1), B)


def lprob_rows(loc, target, scale=0.75, laplace=False, perm_c=0):
    x, t = _paired(loc, target, perm_c)
    lap = row_is_laplace(x.shape[0], laplace)[:, None]
    return torch.where(lap, lprob_elems(x, t, scale, True), lprob_elems(x, t, scale, False)).sum(-1)


def lprob_rows_dloc(loc, target, g_row, scale=0.75, laplace=False, perm_c=0, logit_grad=False):
    """gradient of lprob_rows in loc's own memory layout; logit_grad: loc = sigmoid(logits), gradient wrt the logits"""
    x, t = _paired(loc, target, perm_c)
    B, F_ = x.shape
    lap = row_is_laplace(B, laplace)[:, None]
    v = torch.where(lap, lprob_velems(x, t, scale, True), lprob_velems(x, t, scale, False))
    if logit_grad:
        v = v * x.double() * (1.0 - x.double())
    v = g_row.double()[:, None] * v
    if perm_c:
        v = v.reshape(B, F_ // perm_c, perm_c).transpose(1, 2).reshape(B, F_)
    return v.reshape(loc.shape)


def lprob_elem_fwd(loc, target, scale, laplace):
    """flat loc (n,) against a target of n / k elements that repeats"""
    return lprob_elems(loc, target.repeat(loc.numel() // target.numel()), scale, laplace)


def lprob_elem_dloc(loc, target, g, scale, laplace):
    return g.double() * lprob_velems(loc, target.repeat(loc.numel() // target.numel()), scale, laplace)


# ---------------------------------------------------------------------------------------------
# optimal_sigma (objectives.py:503-509): ONE log sigma = softclip(log sqrt(mean (t - x)^2), -6) per call; the squared
# term is detached, so log sigma is the only gradient path
# ---------------------------------------------------------------------------------------------
def optsig_stats(loc, target, dtype=F64):
    """(mean square, log sigma, raw log sigma) computed in `dtype`"""
    d = target.to(dtype) - loc.to(dtype)
    msq = (d * d).mean()
    raw = 0.5 * torch.log(msq)
    return torch.stack([msq, -6.0 + F.softplus(raw + 6.0), raw])


def optsig_elems(loc, target):
    _, ls, _ = optsig_stats(loc, target)
    q = (target.double() - loc.double()) * torch.exp(-ls)
    return q * q + ls + HALF_LOG_2PI


def optsig_rows(loc, target):
    return optsig_elems(loc, target).reshape(loc.shape[0], -1).sum(-1)


def optsig_dloc(loc, target, g_sum):
    """g_sum = the sum of the upstream gradient over every ELEMENT (rows form: F * sum_b g_b):
    d log_sigma / d raw = sigmoid(raw + 6), d raw / d x_i = -(t_i - x_i) / (n msq)"""
    msq, _, raw = optsig_stats(loc, target)
    d = target.double() - loc.double()
    return -float(g_sum) * torch.sigmoid(raw + 6.0) / (d.numel() * msq) * d


# ---------------------------------------------------------------------------------------------
# l1 / mse (objectives.py:427-459): kind 0 = |x - t|, 1 = (x - t)^2
# ---------------------------------------------------------------------------------------------
def pw_elems(x, target, kind):
    d = x.double() - target.double()
    return d * d if kind else d.abs()


def pw_grad(x, target, kind):
    d = x.double() - target.double()
    return 2.0 * d if kind else torch.sign(d)            # sign(0) = 0


def pw_rows(x, target, kind):
    B = x.shape[0]
    return pw_elems(x.reshape(B, -1), repeat_rows(target.reshape(target.shape[0], -1), B), kind).sum(-1)


def pw_rows_dx(x, target, g_row, kind):
    B = x.shape[0]
    return g_row.double()[:, None] * pw_grad(x.reshape(B, -1), repeat_rows(target.reshape(target.shape[0], -1), B), kind)


# ---------------------------------------------------------------------------------------------
# ELBO assembly: out[k] = sum_n W[k][n] sum_b V[n][b]
# ---------------------------------------------------------------------------------------------
def lincomb(V, W):
    return torch.as_tensor(W, dtype=F64) @ V.double().sum(1)


def lincomb_dV(W, g, B):
    """g: one upstream value per output, None = that output is not part of the backward"""
    gv = torch.tensor([0.0 if x is None else float(x) for x in g], dtype=F64)
    return (gv @ torch.as_tensor(W, dtype=F64))[:, None].expand(-1, B)


# =============================================================================================
# inputs: one deterministic builder per family, shared by the GPU tests and the host test
# =============================================================================================
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# F: 1, 3, 37, 1027 scalar path | 4, 784 float4 tail only | 1028 tail with two passes for thread 0 and a second
# grid.y chunk of one float4 in bce_bwd_kernel | 3600 threads 0-131 in the unrolled main loop, the rest tail only |
# 4096 one main round, no tail | 4100 main round + one tail element, bce_rowsum_bwd past its 16-chunk cap
BCE_WIDTHS = (1, 3, 37, 1027, 4, 784, 1028, 3600, 4096, 4100)
BCE_BATCHES = ((1, 1), (5, 5), (6, 2), (6, 3))           # (B, target rows)
ELEM_SIZES = (1, 255, 257, CAP + 3)


@functools.lru_cache(maxsize=None)
def bce_case(B, F_, trows):
    """logits 6 randn with +-20 / +-50 planted (clamp active), uniform targets with a block of exact 0 / 1"""
    g = _gen(B, F_, trows, 1)
    n, tn = B * F_, trows * F_
    logit = (6.0 * torch.randn(n, generator=g))
    target = torch.rand(tn, generator=g)
    blk = max(1, tn // 8)
    target[:blk] = (torch.arange(blk) % 2).float()
    # four saturated logits, each on the WRONG side of its target (a saturated logit on the right side of an exact
    # target is a term of 1e-6, and a one-element row of it would be a row sum at the noise floor); element 0 is +20
    # against an exact 0, the second one -20 against an exact 1
    where = [(k * n) // 4 for k in range(4)]
    pos = lambda i: (i // F_ % trows) * F_ + i % F_      # the target element paired with output element i
    if pos(where[1]) != pos(where[0]):
        target[pos(where[1])] = 1.0
    for i, mag in reversed(list(zip(where, (20.0, 20.0, 50.0, 50.0)))):
        logit[i] = mag if float(target[pos(i)]) < 0.5 else -mag
    logit = logit.reshape(B, F_)
    x_hat = torch.sigmoid(logit).clamp(1e-6, 1.0 - 1e-6)
    return {"logit": logit, "x_hat": x_hat, "target": target.reshape(trows, F_),
            "g_row": torch.randn(B, generator=g), "dy": torch.randn(B, F_, generator=g)}


def bce_raw_case(F_):
    """raw x_hat of exactly 0 and 1 against t in {0, 1, 0.3}: the -100 clamp of both logs (forward only)"""
    x = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]).repeat(F_ // 6 + 1)[:F_]
    t = torch.tensor([0.0, 1.0, 0.3, 0.0, 1.0, 0.3]).repeat(F_ // 6 + 1)[:F_]
    return torch.stack([x, x.flip(0)]), torch.stack([t, t])


# (T, V): (1,1), (1,27) softmax over a single step | (45,27) workload | (64,64), (16,256) tile kernel at both limits |
# (152,27) n = 4104, fall-back by size | (16,257), (3,300) fall-back by V, five lane passes
CE_SHAPES = ((1, 1), (1, 27), (45, 27), (64, 64), (16, 256), (152, 27), (16, 257), (3, 300))
CE_TILE_SHAPES = CE_SHAPES[:5]
CE_CASES = tuple((B, T, V, tr) for T, V in CE_SHAPES for B in (1, 4) for tr in sorted({B, max(1, B // 2)}))


@functools.lru_cache(maxsize=None)
def ce_case(B, T, V, trows):
    """logits 2 randn; column 0 alternates +-80 over time, column V-1 holds equal logits, and (from V = 3 on) column 1
    alternates +-100 the same way: e^80 = 5.5e34 is still a float32, e^100 is not, so this is the column that overflows exp unless the
    maximum is subtracted.  One-hot targets; every row has a token in each planted column; the last target row ends in
    padded steps (all-zero target), as the text batches do."""
    g = _gen(B, T, V, trows, 2)
    logits = 2.0 * torch.randn(B, T, V, generator=g)
    alt = torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0)
    logits[:, :, 0] = 80.0 * alt
    if V >= 2:
        logits[:, :, V - 1] = 0.7
    if V >= 3:
        logits[:, :, 1] = 100.0 * alt
    tok = torch.randint(0, V, (trows, T), generator=g)
    tok[:, 0] = 0
    if T > 1 and V >= 3:
        tok[:, 1] = 1
    if T > 2 and V >= 2:
        tok[:, 2] = V - 1
    target = F.one_hot(tok, V).float()
    target[trows - 1, T - max(1, T // 4):] = 0.0
    return {"logits": logits, "target": target, "g": torch.randn(B, V, generator=g),
            "g_row": torch.randn(B, generator=g)}


LPROB_WIDTHS = (1, 255, 300, 771)                        # 771 = 3 * 257: a perm_c plane one past a workgroup
LPROB_B = 6
LPROB_MASK = (0b10, 3)                                   # rows 0-2 Normal, rows 3-5 Laplace


def lprob_perm_c(F_):
    return 3 if F_ % 3 == 0 else 1


@functools.lru_cache(maxsize=None)
def lprob_case(F_, kind):
    """kind "mask": fixed scale, full target | "ksample": loc = sigmoid(logits) as (B, perm_c, F / perm_c) planes
    against a 3-row target | "own": scale := loc with negative locations (NaN -> 0)"""
    g = _gen(F_, len(kind), 3)
    B = LPROB_B
    if kind == "ksample":
        loc = torch.sigmoid(1.5 * torch.randn(B, F_, generator=g))
        target = torch.rand(3, F_, generator=g)
    else:
        loc = 0.7 * torch.randn(B, F_, generator=g)
        target = torch.randn(B, F_, generator=g)
    if kind == "own":
        loc[0, 0], loc[1, 0] = -0.5, 0.8
    return {"loc": loc, "target": target, "g_row": torch.randn(B, generator=g)}


LPROB_ELEM_N = CAP + 4        # divisible by 3 (CAP + 3 is not: the library refuses a target that does not repeat evenly)


@functools.lru_cache(maxsize=None)
def lprob_elem_case(n, tn, own):
    g = _gen(n, tn, own, 4)
    loc = 0.7 * torch.randn(n, generator=g)
    return {"loc": loc, "target": torch.randn(tn, generator=g), "g": torch.randn(n, generator=g).double()}


PW_WIDTHS = (1, 255, 256, 257, 4100)                     # 4100: pointwise_rowsum_bwd past its 16-chunk cap
PW_BATCHES = ((6, 2), (6, 3))


@functools.lru_cache(maxsize=None)
def pw_case(B, F_, trows):
    """exact ties x == t wherever (row + column) % 5 == 0"""
    g = _gen(B, F_, trows, 5)
    x = torch.randn(B, F_, generator=g)
    target = torch.randn(trows, F_, generator=g)
    tie = (torch.arange(B)[:, None] + torch.arange(F_)[None, :]) % 5 == 0
    x = torch.where(tie, repeat_rows(target, B), x)
    return {"x": x, "target": target, "tie": tie, "g_row": torch.randn(B, generator=g)}


@functools.lru_cache(maxsize=None)
def pw_elem_case(n):
    g = _gen(n, 6)
    x, target = torch.randn(n, generator=g), torch.randn(n, generator=g)
    tie = torch.arange(n) % 5 == 0
    return {"x": torch.where(tie, target, x), "target": target, "tie": tie, "g": torch.randn(n, generator=g)}


# (3, 1 400 000): n = 4.2 M > 4096 * 1024, so the partial count is capped at 1024 and every partial block strides
OPTSIG_SHAPES = ((1, 1), (3, 4097), (3, 1400000))


@functools.lru_cache(maxsize=None)
def optsig_case(B, F_):
    g = _gen(B, F_, 7)
    return {"loc": 0.7 * torch.randn(B, F_, generator=g), "target": torch.randn(B, F_, generator=g),
            "g_row": torch.randn(B, generator=g), "g": torch.randn(B, F_, generator=g)}


LINCOMB_SHAPES = ((1, 1, 1), (32, 4, 257), (7, 2, 1000))  # (n_rows, n_out, B); 32 and 4 are LC_MAX_ROWS / LC_MAX_OUT


@functools.lru_cache(maxsize=None)
def lincomb_case(n_rows, n_out, B):
    g = _gen(n_rows, n_out, B, 8)
    W = torch.randn(n_out, n_rows, generator=g)
    return {"V": torch.randn(n_rows, B, generator=g), "W": [[float(v) for v in row] for row in W],
            "g": [float(v) for v in torch.randn(n_out, generator=g)]}


def lincomb_split(n_rows, mixed):
    """the rows as blocks: every row a (B,) tensor, or (r, B) tensors around one (B,) tensor (0 = a (B,) tensor,
    r = an (r, B) one)"""
    if not mixed:
        return [0] * n_rows
    if n_rows == 1:
        return [1]
    a = (n_rows - 1) // 2
    return [a, 0, n_rows - 1 - a]
