"""What tests/test_attention_gpu.py measures the attention kernels (csrc/text.hip: mmvae_attn_fwd / mmvae_attn_bwd) against:
a float64 restatement of the op written out from its definition, the case table with the kernel every case is meant to
reach, the deterministic inputs of every case, and the part-by-part comparison.  tests/test_attention_reference_host.py
pins the restatement to torch on the CPU, the case table to the library's own selector (mmvae_attn_path) and the
tolerances to the float32 evaluation of the restatement.

The op (nn.MultiheadAttention's core, identity projections): q (L, N, E), k, v (S, N, E), E = H hd, head h = columns
[h hd, (h + 1) hd).  score[n,h,l,s] = q[l,n,h] . k[s,n,h] / sqrt(hd), -inf where key s of sample n is ignored;
probs = softmax over s; out[l,n,h] = sum_s probs m v[s,n,h] with the dropout multiplier m (0 or 1 / (1 - p)) of element
((n H + h) L + l) S + s.  A sample without any valid key is NaN throughout (0 / 0), as torch gives it."""
import math
import zlib

import torch

F64 = torch.float64
PARTS = ("out", "probs", "dq", "dk", "dv")
GRADS = ("dq", "dk", "dv")
# of each part's own float64 maximum: what tests/test_hip_ops.py always asked of `out` and of the packed gradient
CAP = {"out": 2e-5, "probs": 2e-5, "dq": 5e-5, "dk": 5e-5, "dv": 5e-5}
# Worst error of THIS restatement evaluated in float32 on the CPU against its float64 evaluation, per part on the part's own
# maximum, over the whole case table, rounded up by about 15 % (test_attention_reference_host.
# test_float32_restatement_errors re-measures and asserts them; measured: out 5.42e-6, probs 7.92e-6, dq 1.54e-5,
# dk 4.03e-6, dv 4.38e-6).  The padded-key cases set all five: a float32 score near -40 is good to 3.8e-6 per rounding and
# a softmax weight moves by p (1 - p) times the error of a score difference.  Everywhere else the figure is below 1e-6.
F32_ERR = {"out": 6.0e-6, "probs": 9.0e-6, "dq": 1.8e-5, "dk": 4.6e-6, "dv": 5.0e-6}
MARGIN = 8.0        # different summation order, fp32 MFMA accumulation, __expf in the transposed forward


def tol(part):
    """the GPU tolerance of a part: 8x the float32 restatement's own error, never looser than CAP"""
    return min(MARGIN * F32_ERR[part], CAP[part])


def ignored_keys(mask, mask_is_valid):
    """(N, S) bool, True = key takes no part; any non-zero byte counts as set"""
    return (mask != 0) != bool(mask_is_valid)


def attention_reference(q, k, v, H, mask=None, mask_is_valid=False, mult=None, dout=None):
    """-> dict out (L, N, E), probs (N, H, L, S) normalised and pre-dropout, and with dout: dq, dk, dv; in the dtype of q"""
    L, N, E = q.shape
    S = k.shape[0]
    assert k.shape == (S, N, E) and v.shape == (S, N, E) and E % H == 0
    hd = E // H
    scale = 1.0 / math.sqrt(hd)
    qh = q.reshape(L, N, H, hd).permute(1, 2, 0, 3)
    kh = k.reshape(S, N, H, hd).permute(1, 2, 0, 3)
    vh = v.reshape(S, N, H, hd).permute(1, 2, 0, 3)
    score = torch.einsum("nhld,nhsd->nhls", qh * scale, kh)
    if mask is not None:
        assert mask.shape == (N, S)
        score = score.masked_fill(ignored_keys(mask, mask_is_valid)[:, None, None, :], float("-inf"))
    e = torch.exp(score - score.max(-1, keepdim=True).values)      # all keys ignored: -inf - -inf = NaN
    probs = e / e.sum(-1, keepdim=True)
    m = torch.ones_like(probs) if mult is None else mult.to(q.dtype).reshape(N, H, L, S)
    pm = probs * m
    res = {"out": torch.einsum("nhls,nhsd->nhld", pm, vh).permute(2, 0, 1, 3).reshape(L, N, E), "probs": probs}
    if dout is not None:
        doh = dout.reshape(L, N, H, hd).permute(1, 2, 0, 3)
        dp = torch.einsum("nhld,nhsd->nhls", doh, vh) * m
        ds = probs * (dp - (probs * dp).sum(-1, keepdim=True))
        res["dv"] = torch.einsum("nhls,nhld->nhsd", pm, doh).permute(2, 0, 1, 3).reshape(S, N, E)
        res["dq"] = (torch.einsum("nhls,nhsd->nhld", ds, kh) * scale).permute(2, 0, 1, 3).reshape(L, N, E)
        res["dk"] = (torch.einsum("nhls,nhld->nhsd", ds, qh) * scale).permute(2, 0, 1, 3).reshape(S, N, E)
    return res


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
# kernel instantiations, by the names of include/mmvae_hip.h's enum without the MMVAE_ATTN_ prefix
PATHS = ("ROW_FWD_64_16", "ROW_FWD_64_32", "ROW_FWD_128_16", "ROW_FWD_128_32", "MFMA_FWD", "T_FWD",
         "ROW_BWD_64_16", "ROW_BWD_64_32", "ROW_BWD_128_16", "ROW_BWD_128_32", "MFMA_BWD", "T_BWD")
PATH_VALUE = {name: 16 + i for i, name in enumerate(PATHS)}
# built but served by no supported shape: head_dim <= 16 past 32 rows or keys is an MFMA shape (attn_use_mfma), and up to
# 32 x 32 the 64-thread form runs (test_attention_reference_host sweeps the whole domain of the selector to show it)
UNREACHABLE = ("ROW_FWD_128_16", "ROW_BWD_128_16")
ERR_ARG, ERR_UNSUPPORTED = 1, 2

LAYOUTS = ("packed", "separate", "ld_odd", "offset_base", "offset_probs")
MASKS = ("null", "all_valid", "one_first", "one_last", "first_masked", "scatter", "bytes", "full_sample")
VALUES = ("o1", "pad40", "big", "row1e4")
FULLY_MASKED = 1          # the sample of a "full_sample" case without any valid key


class Case:
    """one input recipe and the kernels it is meant to reach: fwd, and bwd = (with mmvae_attn_t_bwd_set(0), with 1)"""

    def __init__(self, L, S, hd, fwd, bwd, N=3, H=2, layout="separate", mask="scatter", valid=False, values="o1", p=0.1):
        assert layout in LAYOUTS and mask in MASKS and values in VALUES and fwd in PATHS
        bwd = (bwd, bwd) if isinstance(bwd, str) else tuple(bwd)
        assert bwd[0] in PATHS and bwd[1] in PATHS
        assert layout != "packed" or L == S
        assert layout != "offset_probs" or S % 4 == 0
        assert mask != "full_sample" or N > FULLY_MASKED + 1
        assert mask != "first_masked" or S > 1
        self.L, self.S, self.hd, self.N, self.H, self.E = L, S, hd, N, H, H * hd
        self.fwd, self.bwd, self.layout, self.mask, self.valid, self.values, self.p = fwd, bwd, layout, mask, valid, values, p
        self.name = (f"{L}x{S}-hd{hd}-H{H}-N{N}-{layout}-{mask}{'-valid' if valid else ''}-{values}-p{p}")

    def geometry(self):
        """-> ldq, ldk, ldv, base offset of q / k / v (floats), offset of probs (floats); the gradients use the same
        leading dimensions and offsets as their inputs.  packed: one (L, N, 3E) buffer, q | k | v side by side"""
        E = self.E
        if self.layout == "packed":
            return 3 * E, 3 * E, 3 * E, 0, 0
        if self.layout == "ld_odd":
            return E + 1, E + 2, E + 3, 0, 0
        ld = (E + 4, E + 8, E + 12)
        return ld + ((1, 0) if self.layout == "offset_base" else (0, 1) if self.layout == "offset_probs" else (0, 0))

    def aligned16(self):
        """do the pointers the float4 paths inspect sit on 16 bytes (arenas start 16-byte aligned)"""
        if self.layout == "packed":
            return self.E % 4 == 0
        return self.layout != "offset_base"

    @property
    def expressible(self):
        """ops.attention can make this very call: self-attention on a packed buffer"""
        return self.layout == "packed"

    def __repr__(self):
        return self.name


def _row(L, S, hd, am, **kw):
    w = 16 if hd <= 16 else 32
    return Case(L, S, hd, f"ROW_FWD_{am}_{w}", f"ROW_BWD_{am}_{w}", **kw)


def _t(L, S, hd, **kw):
    """MFMA shape, head_dim a multiple of 4, aligned: transposed forward; the register-form backward when switched on"""
    return Case(L, S, hd, "T_FWD", ("MFMA_BWD", "T_BWD"), **kw)


def _mfma(L, S, hd, **kw):
    """MFMA shape that the float4 kernels refuse (head_dim, leading dimension or alignment): the LDS-tile kernels"""
    return Case(L, S, hd, "MFMA_FWD", "MFMA_BWD", **kw)


def _pids(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


# (L, S, an MFMA shape at head_dim <= 16: L > 32 or S > 32, threads of the thread-per-row form: 64 up to 64 x 64)
SHAPES = [(1, 1, False, 64), (1, 7, False, 64), (7, 1, False, 64), (5, 32, False, 64), (32, 5, False, 64),
          (32, 33, True, 64), (33, 5, True, 64), (33, 100, True, 128), (100, 33, True, 128), (64, 65, True, 128),
          (65, 64, True, 128), (97, 128, True, 128), (128, 97, True, 128), (127, 127, True, 128), (128, 128, True, 128)]
SHAPES_HD32 = [(64, 64, True, 64), (65, 3, True, 128)]       # head_dim > 16 only: the AM = 64 -> 128 switch
LT, GT = (33, 100), (100, 33)                                  # the MFMA shapes the sweeps below sit on, L < S and L > S
SMALL = ((5, 32), (32, 5))


def _family(L, S, fam, mfma, am, **kw):
    """fam: 't' (hd 16), 'm' (hd 15), 'r' (hd 27) unless kw names hd"""
    hd = kw.pop("hd", {"t": 16, "m": 15, "r": 27}[fam])
    if hd > 16 or not mfma:
        return _row(L, S, hd, am, **kw)
    return _t(L, S, hd, **kw) if fam == "t" else _mfma(L, S, hd, **kw)


def _build():
    cs = []
    # every shape on every kernel family it can reach
    for L, S, mfma, am in SHAPES:
        for fam in "tmr":
            cs.append(_family(L, S, fam, mfma, am))
    for L, S, mfma, am in SHAPES_HD32:
        cs.append(_row(L, S, 27, am))
        cs.append(_row(L, S, 17, am, H=1, p=0.0))
    # head dims and head counts
    for (L, S) in (LT, GT):
        for hd, H in ((12, 2), (8, 4), (4, 1)):
            cs.append(_t(L, S, hd, H=H))
        for hd, H in ((10, 2), (6, 4), (1, 1)):
            cs.append(_mfma(L, S, hd, H=H))
        for hd, H in ((17, 1), (32, 2), (27, 4)):
            cs.append(_row(L, S, hd, 128, H=H))
    for (L, S) in SMALL:
        for hd, H in ((12, 4), (1, 2), (17, 2), (32, 1)):
            cs.append(_row(L, S, hd, 64, H=H))
    # layouts
    for (L, S) in (LT, GT):
        cs.append(_mfma(L, S, 16, layout="ld_odd"))          # hd 16 on a leading dimension that is no multiple of 4
        cs.append(_mfma(L, S, 16, layout="offset_base"))     # aligned16 = 0 with hd 16
        cs.append(_mfma(L, S, 15, layout="offset_base"))
        cs.append(_row(L, S, 27, 128, layout="ld_odd"))
        cs.append(_row(L, S, 32, 128, layout="offset_base"))
    for (L, S) in SMALL:
        for hd in (16, 32):
            cs.append(_row(L, S, hd, 64, layout="ld_odd"))
            cs.append(_row(L, S, hd, 64, layout="offset_base"))
    for (L, S) in ((33, 100), (65, 64), (97, 128), (128, 128)):       # S % 4 == 0 with a probs pointer off by one float
        cs.append(_t(L, S, 16, layout="offset_probs"))
        cs.append(_mfma(L, S, 15, layout="offset_probs"))
    cs.append(_row(5, 32, 16, 64, layout="offset_probs"))
    cs.append(_row(65, 64, 27, 128, layout="offset_probs"))
    for L, hd, H in ((1, 16, 2), (1, 27, 2), (32, 16, 2), (32, 27, 2), (64, 27, 2), (127, 16, 2), (128, 16, 2),
                     (128, 27, 2), (100, 16, 2)):
        cs.append(_family(L, L, "t", L > 32, 64 if L <= 64 else 128, hd=hd, H=H, layout="packed", p=0.1))
    cs.append(_mfma(127, 127, 15, layout="packed"))          # packed with E = 30: k and v start off 16 bytes
    cs.append(_mfma(100, 100, 6, H=1, layout="packed"))      # ... E = 6, leading dimension 18
    # masks, both polarities on every kernel family
    for i, mask in enumerate(MASKS):
        for j, ((L, S), fam) in enumerate([(LT, "t"), (GT, "t"), (LT, "m"), (GT, "m"), (LT, "r"), (GT, "r"),
                                           (SMALL[0], "t"), (SMALL[1], "r")]):
            if mask == "scatter" and (i + j) % 2 == 0:
                continue                                       # (the shape sweep above has it in this polarity)
            mfma, am = (True, 128) if j < 6 else (False, 64)
            cs.append(_family(L, S, fam, mfma, am, mask=mask, valid=(i + j) % 2 == 1))
    # values
    for L, S, mfma, am in SHAPES + SHAPES_HD32[1:]:
        if S % 32 == 0:
            continue                                           # no padded key in any 32-wide tile
        if (L, S) == (65, 3):
            cs.append(_row(L, S, 27, am, values="pad40"))
            continue
        cs.append(_family(L, S, "t", mfma, am, values="pad40"))
        if mfma:
            cs.append(_family(L, S, "m", mfma, am, values="pad40"))
            cs.append(_mfma(L, S, 16, values="pad40", layout="ld_odd", mask="null"))
    for (L, S) in (LT, GT):
        for fam in "tmr":
            cs.append(_family(L, S, fam, True, 128, values="row1e4"))
        # (big: head dims with an exact 1 / sqrt(hd) only, see make_inputs; MFMA_FWD through the leading dimension)
        cs.append(_t(L, S, 16, values="big"))
        cs.append(_t(L, S, 4, H=4, values="big"))
        cs.append(_mfma(L, S, 16, values="big", layout="ld_odd"))
        cs.append(_mfma(L, S, 4, values="big", layout="offset_base"))
    for (L, S) in SMALL:
        cs.append(_row(L, S, 16, 64, values="row1e4"))
        cs.append(_row(L, S, 16, 64, values="big"))
        cs.append(_row(L, S, 4, 64, values="big", H=1))
    cs.append(_row(64, 64, 27, 64, values="row1e4"))
    # dropout: none, heavy; S odd and L S odd (the odd-index branch of the transposed forward's pair hash)
    for p in (0.0, 0.5):
        for (L, S) in (LT, GT, (127, 127), (97, 128), (128, 97)):
            cs.append(_t(L, S, 16, p=p))
            cs.append(_mfma(L, S, 15, p=p))
        for (L, S) in ((1, 7), (7, 1), (5, 32), (32, 5)):
            cs.append(_row(L, S, 16, 64, p=p))
        cs.append(_row(65, 3, 27, 128, p=p))
    cs.append(_t(127, 127, 12, p=0.1, H=1, N=1))             # N H L S odd
    # batch
    cs.append(_t(33, 100, 16, N=130))
    cs.append(_mfma(100, 33, 15, N=1))
    cs.append(_row(32, 5, 27, 64, N=130))
    cs.append(_row(5, 32, 16, 64, N=1))
    return _pids(cs)


CASES = _build()
LIMIT_CASES = [(129, 5, 16), (5, 129, 16), (129, 129, 16), (5, 5, 33), (128, 128, 33)]        # (L, S, hd): refused


def make_inputs(c):
    """float32 CPU tensors of case c from ONE generator seeded by the case's name: q (L, N, E), k, v (S, N, E), dout,
    mask (N, S) uint8 or None, and a stand-in dropout multiplier (N, H, L, S) for the host tests (the GPU tests read the
    kernels' own from ops.dropout_mask)"""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    L, S, N, H, hd, E = c.L, c.S, c.N, c.H, c.hd, c.E
    q = torch.randn(L, N, E, generator=g)
    k = torch.randn(S, N, E, generator=g)
    v = torch.randn(S, N, E, generator=g)
    dout = torch.randn(L, N, E, generator=g)
    if c.values == "pad40":
        # every real score is -40 + O(1): q = a + noise, k = -a + noise per head with hd a^2 / sqrt(hd) = 40.  A padded
        # key (zero row: score 0) that reached the softmax would outweigh all of them by e^40
        a = math.sqrt(40.0 / math.sqrt(hd))
        q, k = a + 0.05 * q, -a + 0.05 * k
    elif c.values == "big":
        # score = O(1) part + 160 r_l: the second term is constant over the keys of a row (softmax-invariant), of either
        # sign over the rows -- q carries 160 sqrt(hd) r_l, r_l = +-1, along the head's first coordinate and k carries 1 there
        # (not the other way round: dq = sum_s dS K would then be 640 times a sum that cancels to rounding error).
        # A float32 score of magnitude 160 is only good to 1.5e-5 (one ulp) PER ROUNDING, which no kernel can avoid and
        # which alone moves the weights by more than today's bound; so these inputs are made exact instead: head_dim 4 or
        # 16 (1 / sqrt(hd) a power of two) and every entry a multiple of 1 / 8 in [-3, 3], so that every product and every
        # partial sum of a score, in any order, with q scaled before or after, is a float32 number.  What is left is
        # what the case is about: the row maximum has to come off before the exponential.
        assert hd in (4, 16)
        r = torch.where(torch.rand(L, N, H, generator=g) < 0.5, -1.0, 1.0)
        q = (torch.round(q * 8) / 8).clamp(-3, 3).reshape(L, N, H, hd).clone()
        k = (torch.round(k * 8) / 8).clamp(-3, 3).reshape(S, N, H, hd).clone()
        q[..., 0] = r * 160.0 * math.sqrt(hd)
        k[..., 0] = 1.0
        q, k = q.reshape(L, N, E), k.reshape(S, N, E)
    elif c.values == "row1e4":
        v[S // 2] *= 1e4
        dout[L // 2] *= 1e4
    mask = None
    if c.mask != "null":
        ign = torch.zeros(N, S, dtype=torch.bool)
        if c.mask == "one_first":
            ign[:, 1:] = True
        elif c.mask == "one_last":
            ign[:, :-1] = True
        elif c.mask == "first_masked":
            ign[:, 0] = True
        elif c.mask in ("scatter", "bytes", "full_sample"):
            ign = torch.rand(N, S, generator=g) < 0.5
            keep = torch.randint(0, S, (N,), generator=g)
            ign[torch.arange(N), keep] = False          # at least one valid key, anywhere
            if c.mask == "full_sample":
                ign[FULLY_MASKED] = True
        set_ = ~ign if c.valid else ign
        byte = torch.ones(N, S, dtype=torch.uint8)
        if c.mask == "bytes":
            byte = torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (N, S), generator=g)]
        mask = torch.where(set_, byte, torch.zeros_like(byte))
    mult = None
    if c.p > 0:
        mult = (torch.rand(N, H, L, S, generator=g) >= c.p).float() / (1.0 - c.p)
    return {"q": q, "k": k, "v": v, "dout": dout, "mask": mask, "mult": mult}


def run_reference(c, inp, dtype=F64, mult="own"):
    mult = inp["mult"] if isinstance(mult, str) else mult
    return attention_reference(inp["q"].to(dtype), inp["k"].to(dtype), inp["v"].to(dtype), c.H, inp["mask"], c.valid,
                               None if mult is None else mult.to(dtype), inp["dout"].to(dtype))


def finite_samples(c):
    """the samples whose results are numbers: all but the fully masked one"""
    return [n for n in range(c.N) if not (c.mask == "full_sample" and n == FULLY_MASKED)]


def by_sample(part, t, samples):
    """the slice of a part that belongs to `samples`: dim 0 of probs, dim 1 of everything else"""
    idx = torch.as_tensor(samples, dtype=torch.long)
    return t.index_select(0 if part == "probs" else 1, idx.to(t.device))


# ---------------------------------------------------------------------------------------------
# part by part
# ---------------------------------------------------------------------------------------------
def abs_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, f"shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if a.numel() == 0:
        return 0.0
    d = (a - b).abs().max()
    return float(d) if bool(d == d) else float("nan")


class Parts:
    """collects (part, error, bound) of one comparison and asserts them together, naming every part that failed.  Every
    part is judged on its OWN float64 maximum; a part whose reference is identically zero on tolerance x `zero_scale`
    (the largest gradient part of the same case).  `worst` (a dict shared by a test module) keeps each kind's worst
    error over the suite."""

    def __init__(self, what, worst=None):
        self.what, self.rows, self.worst = what, [], worst

    def check(self, part, got, ref, tol_, zero_scale=None, kind=None):
        mx = float(ref.detach().abs().max()) if ref.numel() else 0.0
        if mx == 0.0 and zero_scale is not None:
            mx, part = float(zero_scale), part + " [reference identically 0]"
        e = abs_err(got, ref)
        e = e / max(mx, 1e-300) if e != 0.0 else 0.0
        self.rows.append((part, e, tol_))
        if self.worst is not None and kind is not None and math.isfinite(e):
            self.worst[kind] = max(self.worst.get(kind, 0.0), e)
        print(f"{self.what}: {part}: rel err {e:.3e} (bound {tol_:.1e})")
        return e

    def require(self, part, ok, detail=""):
        """an exact condition (sign bits, sentinels, non-finite samples)"""
        self.rows.append((part + (f" [{detail}]" if detail and not ok else ""), 0.0 if ok else float("inf"), 0.0))

    def failed(self):
        return [p for p, e, t in self.rows if not (math.isfinite(e) and e <= t)]

    def done(self):
        bad = [f"{p}: {e:.3e} > {t:.1e}" for p, e, t in self.rows if not (math.isfinite(e) and e <= t)]
        assert not bad, f"{self.what}: " + "; ".join(bad)


def grad_scale(ref, c=None):
    """the largest gradient part of a case (over the samples that are numbers)"""
    s = 0.0
    for p in GRADS:
        t = ref[p] if c is None else by_sample(p, ref[p], finite_samples(c))
        s = max(s, float(t.abs().max())) if t.numel() else s
    return s


def check_forward(parts, c, out, probs_abs, ref, tols=None, prefix=""):
    smp = finite_samples(c)
    for part, got in (("out", out), ("probs", probs_abs)):
        parts.check(prefix + part, by_sample(part, got, smp), by_sample(part, ref[part], smp),
                    (tols or {}).get(part, tol(part)), kind=prefix + part)


def check_signs(parts, c, probs, mult, prefix=""):
    """the saved probabilities carry the dropout decision in their sign bit: set exactly where the multiplier is 0 (-0.0 at
    a masked key that was dropped too), clear everywhere else (+0.0 at a masked key that was kept)"""
    smp = finite_samples(c)
    got = torch.signbit(by_sample("probs", probs.detach().cpu(), smp))
    want = torch.zeros_like(got) if mult is None else by_sample("probs", mult.detach().cpu().reshape(probs.shape), smp) == 0
    n = int((got != want).sum())
    parts.require(prefix + "probs sign bits", n == 0, f"{n} of {got.numel()} differ from (multiplier == 0)")


def check_backward(parts, c, dq, dk, dv, ref, tols=None, prefix=""):
    smp = finite_samples(c)
    zs = grad_scale(ref, c)
    for part, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        parts.check(prefix + part, by_sample(part, got, smp), by_sample(part, ref[part], smp),
                    (tols or {}).get(part, tol(part)), zero_scale=zs, kind=prefix + part)
