"""Every kernel of csrc/optim.hip against the float64 references of tests/optim_reference.py, per element, relative to the
magnitude of the terms that were added (bounds: that module's docstring; they are pinned on the CPU by
tests/test_optim_reference_host.py, not fitted to these kernels).  Every output array of every launch lies between
canaries -- a bit pattern in front of it, behind it and between destination ranges -- that must come back bit for bit.
The largest error seen per quantity is printed at the end of the module (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import optim_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
FB1, FB2 = R.f32(B1), R.f32(B2)
GSCALES = (1.0, 0.5, 1.0 / 3.0)
CANARY = 0x7FA5C3E1          # a quiet NaN with a payload: arithmetic on it never gives these bits back
PAD = 64                     # floats of canary on either side (256 bytes: the array stays 16-byte aligned)
ERR_ARG, ERR_UNSUPPORTED = 1, 2
WORST = {}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest GPU error per quantity (u = 2^-24 of the term scale unless a bound fraction is named):")
    for k in sorted(WORST):
        print(f"  {k}: {WORST[k]:.3f}")


@pytest.fixture(scope="module")
def H(hip_lib):
    from multimodal_vae_comparison_amd import hipops
    return hipops


class Buf:
    """n floats on the device between canaries; `shift` floats off the 16-byte grid"""

    def __init__(self, host, shift=0):
        host = np.ascontiguousarray(host, dtype=np.float32)
        self.n, self.start = host.size, PAD + shift
        self.raw = torch.full((PAD + shift + self.n + PAD,), CANARY, dtype=torch.int32, device=DEV)
        self.t = self.raw[self.start:self.start + self.n].view(torch.float32)
        self.t.copy_(torch.tensor(host))
        self.ptr = self.t.data_ptr()

    def host(self):
        return self.t.cpu().numpy()

    def intact(self):
        return bool((self.raw[:self.start] == CANARY).all()) and bool((self.raw[self.start + self.n:] == CANARY).all())


def canary_floats(n):
    return np.full(n, CANARY, np.int32).view(np.float32).copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Block:
    """the device step block {count, ticket, beta1^count, beta2^count} between canaries"""

    def __init__(self, count, r1=0.0, r2=0.0):
        self.raw = torch.full((PAD + 6 + PAD,), CANARY, dtype=torch.int32, device=DEV)
        self.raw[PAD:PAD + 2] = torch.tensor([count, 0], dtype=torch.int32)
        self.raw[PAD + 2:PAD + 6].view(torch.float64).copy_(torch.tensor([r1, r2], dtype=torch.float64))
        self.ptr = self.raw[PAD:].data_ptr()

    def read(self):
        c = self.raw[PAD:PAD + 2].tolist()
        r = self.raw[PAD + 2:PAD + 6].view(torch.float64).tolist()
        assert bool((self.raw[:PAD] == CANARY).all()) and bool((self.raw[PAD + 6:] == CANARY).all()), "step block canaries"
        return c[0], c[1], r[0], r[1]


def step_mode(mode, step):
    """(step argument, device block or None, check of the block afterwards) for a launch that must compute `step`"""
    if mode == "explicit":
        return step, None, lambda b: True
    if mode == "block":          # step = 0: read the block, leave it alone
        return 0, Block(step), lambda b: b.read() == (step, 0, 0.0, 0.0)
    if mode == "fresh":
        assert step == 1
        blk = Block(0)
    elif mode == "resumed":      # what FlatAdam.load_state_dict leaves: a count, zeroed running powers -> pow()
        blk = Block(step - 1)
    else:                        # "running": one multiplication by beta
        blk = Block(step - 1, FB1 ** (step - 1), FB2 ** (step - 1))

    def after(b):
        c, tk, r1, r2 = b.read()
        return (c, tk) == (step, 0) and abs(r1 / FB1 ** step - 1) <= 1e-12 and abs(r2 / FB2 ** step - 1) <= 1e-12
    return -1, blk, after


def within(res, ref, bound, what, scale=None, key=None):
    err = np.abs(res.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = np.flatnonzero(bad)
        raise AssertionError(f"{what}: {i.size} of {err.size} elements outside the bound, first {i[:6].tolist()} last "
                             f"{i[-3:].tolist()}: got {res[i[:3]]}, reference {ref[i[:3]]}, bound {bound[i[:3]]}")
    if key is not None:
        sc = bound if scale is None else scale * R.U
        with np.errstate(divide="ignore", invalid="ignore"):
            note(key, np.nanmax(np.where(sc > 0, err / sc, 0.0)))


@functools.lru_cache(maxsize=4)
def adam_case(n, state):
    case = R.adam_case(n, state)
    for a in case:
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=4)
def belief_case(n, state):
    case = R.belief_case(n, state)
    for a in case:
        a.setflags(write=False)
    return case


# ---- Adam (amsgrad) ------------------------------------------------------------------------------------------------------
def check_adam(case, out, step, gs, zg, what, g_ref=None, g_err=None, lo=0, hi=None, frozen=None, tag=""):
    """out: host (p, g, m, v, vmax) after one launch over [lo, hi) that had `case` as input; frozen: what the arrays held
    outside [lo, hi) before the launch (`case` unless an earlier launch of the step has been there)"""
    p0, g0, m0, v0, x0 = case
    hi = p0.size if hi is None else hi
    sl = slice(lo, hi)
    gin = g0 if g_ref is None else g_ref
    ref = R.adam_amsgrad_step(p0[sl], gin[sl], m0[sl], v0[sl], x0[sl], LR, B1, B2, EPS, step, gs)
    bd = R.adam_bounds(p0[sl], gin[sl], m0[sl], v0[sl], x0[sl], LR, B1, B2, EPS, step, gs,
                       g_err=None if g_err is None else g_err[sl])
    P, G, M, V, X = (a[sl] for a in out)
    if g_err is not None:      # the bound carries the folded gradient's own error: report the fraction of it
        within(M, ref[1], bd["m"], f"{what}: m", None, "fold + adam m, fraction of its bound")
        within(V, ref[2], bd["v"], f"{what}: v", None, "fold + adam v, fraction of its bound")
        within(X, ref[3], bd["vmax"], f"{what}: vmax", None, "fold + adam vmax, fraction of its bound")
        within(P, ref[0], bd["p"], f"{what}: p", None, "fold + adam p, fraction of its bound")
    else:
        within(M, ref[1], bd["m"], f"{what}: m", bd["Tm"], tag + "adam m")
        within(V, ref[2], bd["v"], f"{what}: v", bd["Tv"], tag + "adam v")
        within(X, ref[3], bd["vmax"], f"{what}: vmax", ref[3], tag + "adam vmax")
        within(P, ref[0], bd["p"], f"{what}: p")
    half = 0.5 * R.ulp32(np.maximum(np.abs(p0[sl].astype(np.float64)), np.abs(ref[0])))
    over = np.maximum(np.abs(P.astype(np.float64) - ref[0]) - half, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if g_err is None:
            note(tag + "adam p beyond 1/2 ulp, u of S", np.nanmax(np.where(bd["S"] > 0, over / (bd["S"] * R.U), 0.0)))
    assert same_bits(X, np.maximum(x0[sl], V)), f"{what}: vmax_out != max(vmax_in, v_out)"
    if zg:
        assert not bits(G).any(), f"{what}: gradient not cleared"
    elif g_ref is None:
        assert same_bits(G, g0[sl]), f"{what}: zero_grad = 0 touched the gradient"
    for name, a, a0 in zip("pgmvx", out, case if frozen is None else frozen):      # outside [lo, hi): bit-untouched
        assert same_bits(a[:lo], a0[:lo]) and same_bits(a[hi:], a0[hi:]), f"{what}: {name} changed outside [{lo}, {hi})"


def run_adam(lib, H, case, mode, step, gs, zg, what, tag=""):
    bufs = [Buf(a) for a in case]
    arg, blk, after = step_mode(mode, step)
    rc = lib.mmvae_adam_amsgrad_flat(*[b.ptr for b in bufs], case[0].size, LR, B1, B2, EPS, arg,
                                     blk.ptr if blk else None, gs, zg, H.stream())
    assert rc == 0, f"{what}: rc {rc}"
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs), f"{what}: canaries"
    assert after(blk), f"{what}: step block {blk.read()}"
    out = [b.host() for b in bufs]
    check_adam(case, out, step, gs, zg, what, tag=tag)
    return bufs, blk, out


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 10007])
def test_adam_per_element(hip_lib, H, n):
    """state x grad_scale x zero_grad, the step-count modes going round; one workgroup (n <= 2048) and five"""
    k = 0
    for state in ("zero", "mid"):
        modes = ("explicit", "block", "fresh") if state == "zero" else ("explicit", "block", "resumed", "running")
        step = 1 if state == "zero" else 42
        for gs in GSCALES:
            for zg in (1, 0):
                mode = modes[k % len(modes)]
                k += 1
                run_adam(hip_lib, H, adam_case(n, state), mode, step, gs, zg, f"n {n} {state} gs {gs:.3g} zg {zg} {mode}")


@pytest.mark.parametrize("state,mode", [("zero", "explicit"), ("zero", "block"), ("zero", "fresh"), ("mid", "explicit"),
                                        ("mid", "block"), ("mid", "resumed"), ("mid", "running")])
def test_adam_every_step_count_mode(hip_lib, H, state, mode):
    run_adam(hip_lib, H, adam_case(10007, state), mode, 1 if state == "zero" else 42, 1.0 / 3.0, 1, f"{state} {mode}")


@pytest.mark.parametrize("state,mode,gs,zg", [("mid", "resumed", 1.0 / 3.0, 1), ("zero", "fresh", 0.5, 0)])
def test_adam_past_the_grid_cap(hip_lib, H, state, mode, gs, zg):
    """n = 2048 * 256 * 8 + 2048 * 4 + 3: the grid is capped at 2048 workgroups, the paired float4 loop iterates, 2048 threads
    take the single-float4 leftover and three elements the dword tail"""
    n = 2048 * 256 * 8 + 2048 * 4 + 3
    run_adam(hip_lib, H, adam_case(n, state), mode, 1 if state == "zero" else 42, gs, zg, f"n {n} {state} {mode}")


def test_adam_resumed_is_step_42_then_43(hip_lib, H):
    """block {41, 0, 0.0, 0.0}: the launch calls pow() and must be torch's step 42; the next one is step 43 through the
    running products it left"""
    case = adam_case(10007, "mid")
    bufs, blk, out = run_adam(hip_lib, H, case, "resumed", 42, 1.0, 0, "resumed")
    rc = hip_lib.mmvae_adam_amsgrad_flat(*[b.ptr for b in bufs], case[0].size, LR, B1, B2, EPS, -1, blk.ptr, 1.0, 0,
                                         H.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs)
    check_adam(out, [b.host() for b in bufs], 43, 1.0, 0, "step 43")
    c, tk, r1, r2 = blk.read()
    assert (c, tk) == (43, 0) and abs(r1 / FB1 ** 43 - 1) <= 1e-12 and abs(r2 / FB2 ** 43 - 1) <= 1e-12


def test_adam_200_self_counting_launches(hip_lib, H):
    bufs = [Buf(a) for a in adam_case(4, "zero")]
    blk = Block(0)
    for _ in range(200):
        assert hip_lib.mmvae_adam_amsgrad_flat(*[b.ptr for b in bufs], 4, LR, B1, B2, EPS, -1, blk.ptr, 1.0, 0,
                                               H.stream()) == 0
    torch.cuda.synchronize()
    c, tk, r1, r2 = blk.read()
    assert (c, tk) == (200, 0)
    assert abs(r1 / FB1 ** 200 - 1) <= 1e-12 and abs(r2 / FB2 ** 200 - 1) <= 1e-12, (r1, r2)
    assert all(b.intact() for b in bufs) and all(np.isfinite(b.host()).all() for b in bufs)


@pytest.mark.parametrize("gval", [0.0, 1e-20, 1e15])
def test_adam_edge_gradients(hip_lib, H, gval):
    n = 37
    p, _, m, v, x = adam_case(n, "zero")
    case = (p, np.full(n, gval, np.float32), m, v, x)
    _, _, out = run_adam(hip_lib, H, case, "explicit", 1, 1.0, 0, f"g = {gval}", tag=f"(g = {gval:g}) ")
    assert all(np.isfinite(a).all() for a in out)
    if gval == 0.0:
        assert same_bits(out[0], p) and not bits(out[2]).any() and not bits(out[3]).any()


def test_adam_refusals_launch_nothing(hip_lib, H):
    case = adam_case(1023, "mid")
    bufs = [Buf(a) for a in case]
    blk = Block(41)
    ptrs = [b.ptr for b in bufs]
    call = lambda pp, n, step, bp: hip_lib.mmvae_adam_amsgrad_flat(*pp, n, LR, B1, B2, EPS, step, bp, 1.0, 1, H.stream())
    for k in range(5):                                      # an unaligned base, each array in turn
        assert call(ptrs[:k] + [ptrs[k] + 4] + ptrs[k + 1:], 1000, 7, None) == ERR_ARG
    assert call(ptrs, 0, 7, None) == ERR_ARG
    assert call(ptrs, 1023, 0, None) == ERR_ARG            # step = 0 without a block
    assert call(ptrs, 1023, -1, None) == ERR_ARG
    assert call(ptrs, 1023, -1, blk.ptr + 4) == ERR_ARG    # the running powers are doubles
    torch.cuda.synchronize()
    assert all(b.intact() and same_bits(b.host(), a) for b, a in zip(bufs, case)) and blk.read() == (41, 0, 0.0, 0.0)


# ---- AdaBelief ------------------------------------------------------------------------------------------------------------
BEPS = 1e-16      # as the trainer sets it


def run_belief(lib, H, case, mode, step, gs, zg, what):
    bufs = [Buf(a) for a in case]
    arg, blk, after = step_mode(mode, step)
    rc = lib.mmvae_adabelief_flat(*[b.ptr for b in bufs], case[0].size, LR, B1, B2, BEPS, arg, blk.ptr if blk else None,
                                  gs, zg, H.stream())
    assert rc == 0, f"{what}: rc {rc}"
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs), f"{what}: canaries"
    assert after(blk), f"{what}: step block {blk.read()}"
    P, G, M, S = (b.host() for b in bufs)
    p0, g0, m0, s0 = case
    ref = R.adabelief_step(p0, g0, m0, s0, LR, B1, B2, BEPS, step, gs)
    bd = R.adabelief_bounds(p0, g0, m0, s0, LR, B1, B2, BEPS, step, gs)
    within(M, ref[1], bd["m"], f"{what}: m", bd["Tm"], "adabelief m")
    within(S, ref[2], bd["s"], f"{what}: s", None, "adabelief s, fraction of its bound")
    within(P, ref[0], bd["p"], f"{what}: p")
    half = 0.5 * R.ulp32(np.maximum(np.abs(p0.astype(np.float64)), np.abs(ref[0])))
    over = np.maximum(np.abs(P.astype(np.float64) - ref[0]) - half, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        note("adabelief p beyond 1/2 ulp, fraction of the rest of its bound",
             np.nanmax(np.where(bd["p_rel"] > 0, over / bd["p_rel"], 0.0)))
    if zg:
        assert not bits(G).any(), f"{what}: gradient not cleared"
    else:
        assert same_bits(G, g0), f"{what}: zero_grad = 0 touched the gradient"


@pytest.mark.parametrize("n", [1, 5, 10007])
def test_adabelief_per_element(hip_lib, H, n):
    k = 0
    for state in ("zero", "mid"):
        modes = ("explicit", "block", "fresh") if state == "zero" else ("explicit", "block", "resumed", "running")
        for gs in GSCALES:
            for zg in (1, 0):
                mode = modes[k % len(modes)]
                k += 1
                run_belief(hip_lib, H, belief_case(n, state), mode, 1 if state == "zero" else 42, gs, zg,
                           f"n {n} {state} gs {gs:.3g} zg {zg} {mode}")


@pytest.mark.parametrize("state,mode", [("zero", "explicit"), ("zero", "block"), ("zero", "fresh"), ("mid", "explicit"),
                                        ("mid", "block"), ("mid", "resumed"), ("mid", "running")])
def test_adabelief_every_step_count_mode(hip_lib, H, state, mode):
    run_belief(hip_lib, H, belief_case(10007, state), mode, 1 if state == "zero" else 42, 0.5, 1, f"{state} {mode}")


@pytest.mark.parametrize("state,mode,gs,zg", [("mid", "resumed", 1.0 / 3.0, 1), ("zero", "fresh", 0.5, 0)])
def test_adabelief_past_the_grid_cap(hip_lib, H, state, mode, gs, zg):
    """n = 2 100 003 > 2048 * 1024: the grid-stride loop iterates"""
    run_belief(hip_lib, H, belief_case(2100003, state), mode, 1 if state == "zero" else 42, gs, zg, f"{state} {mode}")


def test_adabelief_refusals_launch_nothing(hip_lib, H):
    case = belief_case(5, "mid")
    bufs = [Buf(a) for a in case]
    ptrs = [b.ptr for b in bufs]
    call = lambda n, step, bp: hip_lib.mmvae_adabelief_flat(*ptrs, n, LR, B1, B2, BEPS, step, bp, 1.0, 1, H.stream())
    assert call(0, 7, None) == ERR_ARG and call(5, 0, None) == ERR_ARG and call(5, -1, None) == ERR_ARG
    torch.cuda.synchronize()
    assert all(b.intact() and same_bits(b.host(), a) for b, a in zip(bufs, case))


# ---- reduce_rows ------------------------------------------------------------------------------------------------------------
def check_reduce_rows(lib, H, rng, rows, ln, extra):
    stride = ln + extra
    src = np.full(rows * stride, 1e6, np.float32)                   # junk between the rows
    src.reshape(rows, stride)[:, :ln] = rng.standard_normal((rows, ln), dtype=np.float32)
    sm, ab = R.rows_sum(src, rows, ln, stride)
    sbuf = Buf(src)
    d0 = rng.standard_normal(ln, dtype=np.float32)
    for acc in (0, 1):
        dst = Buf(d0 if acc else np.full(ln, np.nan, np.float32))   # accumulate = 0 must not read the destination
        assert lib.mmvae_reduce_rows(sbuf.ptr, dst.ptr, rows, ln, stride, acc, H.stream()) == 0
        torch.cuda.synchronize()
        assert dst.intact() and sbuf.intact(), f"reduce_rows {rows} x {ln} acc {acc}: canaries"
        ref = sm + d0 if acc else sm
        mag = ab + np.abs(d0) if acc else ab
        within(dst.host(), ref, (rows + acc + 1) * R.U * mag + R.TINY, f"reduce_rows {rows} x {ln} stride {stride} acc {acc}",
               mag * (rows + acc + 1), "reduce_rows, fraction of (R + 1) u sum|terms|")
    assert same_bits(sbuf.host(), src)


def test_reduce_rows_per_column(hip_lib, H):
    """row counts on both sides of the unrolled walk's boundary (r + 28 < n_rows) for every row slice; lengths around
    the 64-column block; stride > len; accumulate 0 and 1"""
    rng = np.random.default_rng(21)
    for rows in (1, 3, 4, 28, 29, 32, 33, 61, 100):
        for ln in (1, 63, 64, 65, 1000):
            check_reduce_rows(hip_lib, H, rng, rows, ln, 3)
    check_reduce_rows(hip_lib, H, rng, 5, 64, 0)      # stride == len


def test_reduce_rows_past_4096_workgroups(hip_lib, H):
    check_reduce_rows(hip_lib, H, np.random.default_rng(22), 33, 4096 * 64 + 70, 2)


def test_reduce_rows_refusals(hip_lib, H):
    dst = Buf(np.zeros(8, np.float32))
    src = Buf(np.ones(64, np.float32))
    assert hip_lib.mmvae_reduce_rows(src.ptr, dst.ptr, 0, 8, 8, 0, H.stream()) == ERR_ARG
    assert hip_lib.mmvae_reduce_rows(src.ptr, dst.ptr, 4, 0, 8, 0, H.stream()) == ERR_ARG
    assert hip_lib.mmvae_reduce_rows(None, dst.ptr, 4, 8, 8, 0, H.stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert dst.intact() and not bits(dst.host()).any()


# ---- reduce_segments (+ rider) -----------------------------------------------------------------------------------------------
def lay_out(rng, specs, gaps=None, first=0):
    """specs: (rows of every chain member, len, source aligned, destination aligned, stride % 4 == 0) per destination range
    -> arena (random everywhere: the floats between the rows of a partial region are junk that must not be read),
    segments (src, dst, rows, len, stride) in offsets, a destination array (random inside the ranges, canaries between
    them) and the ranges.  `gaps`: exact distance of every range from the end of the one before (the alignment flag of
    the destination is then ignored); otherwise at least 8 canaries."""
    segs, ranges, so, do = [], [], 0, first
    for k, (chain, ln, sa, da, st4) in enumerate(specs):
        if gaps is not None:
            do += gaps[k]
        else:
            do = (do + 8 + 3) // 4 * 4 + (0 if da else 1 + k % 3)
        for j, rows in enumerate(chain):
            so = (so + 3) // 4 * 4 + (0 if sa else 1 + (k + j) % 3)
            stride = (ln + 3) // 4 * 4 + 4 + (0 if st4 else 1 + (k + j) % 3)
            segs.append((so, do, rows, ln, stride))
            so += rows * stride
        ranges.append((do, do + ln))
        do += ln
    arena = rng.standard_normal(so + 8, dtype=np.float32)
    dst = canary_floats(do + (0 if gaps is not None else 8))
    for a, b in ranges:
        dst[a:b] = rng.standard_normal(b - a, dtype=np.float32)
    return arena, segs, dst, ranges


def table_of(H, segs, arena_ptr, dst_ptr, order=None):
    t = H.ReduceSegments()
    for j, i in enumerate(order if order is not None else range(len(segs))):
        so, do, rows, ln, sd = segs[i]
        t.src[j], t.dst[j], t.rows[j], t.len[j], t.stride[j] = arena_ptr + 4 * so, dst_ptr + 4 * do, rows, ln, sd
    t.n = len(segs)
    return t


def outside(ranges, n):
    mask = np.ones(n, bool)
    for a, b in ranges:
        mask[a:b] = False
    return mask


def check_fold(dst_out, dst0, arena, segs, ranges, what):
    ref, bound = R.fold(np.where(outside(ranges, dst0.size), 0.0, dst0), arena, segs)
    m = ~outside(ranges, dst0.size)
    within(dst_out[m], ref[m], bound[m], what, bound[m] / R.U, "fold, fraction of (R + 1) u sum|terms|")
    assert same_bits(dst_out[~m], dst0[~m]), f"{what}: canaries between the destination ranges"


ALIGN = [(sa, da, st4) for sa in (True, False) for da in (True, False) for st4 in (True, False)]


def segment_specs():
    specs = [([rows], ln, *al) for ln in (1, 2, 3, 255, 256, 257) for rows in (1, 127, 128) for al in ALIGN]
    specs += [([rows], ln, *al) for ln in (63, 64, 65) for rows in (128, 200) for al in ALIGN]      # narrow block edge
    return specs


@pytest.mark.parametrize("part", range(4))
def test_reduce_segments_per_column(hip_lib, H, part):
    """lengths 1, 2, 3, the wide block's edge (255, 256, 257; 1, 127, 128 rows) and the narrow one's (63, 64, 65; >= 128
    rows), every combination of an aligned / unaligned source base, destination base and stride % 4; plus a chain of
    three (5, 130 and 33 rows: the 130 makes the whole head narrow).  The last part fills the table: 64 segments."""
    rng = np.random.default_rng(30 + part)
    specs = segment_specs()[part::4]
    for ln, al in ((64, ALIGN[0]), (65, ALIGN[0]), (256, ALIGN[part]), (100, ALIGN[7 - part])):
        specs.append(([5, 130, 33], ln, *al))
    if part == 3:
        specs += [([2], 7, True, False, True)] * (64 - sum(len(c) for c, *_ in specs))
    arena, segs, dst0, ranges = lay_out(rng, specs)
    assert len(segs) <= 64 and (part != 3 or len(segs) == 64)
    ab, db = Buf(arena), Buf(dst0)
    order = rng.permutation(len(segs)).tolist()          # chain members apart, heads unsorted
    t = table_of(H, segs, ab.ptr, db.ptr, order)
    assert hip_lib.mmvae_reduce_segments(ctypes.byref(t), H.stream()) == 0
    torch.cuda.synchronize()
    assert ab.intact() and db.intact(), "canaries"
    check_fold(db.host(), dst0, arena, segs, ranges, f"reduce_segments part {part}")
    assert same_bits(ab.host(), arena)
    if part == 3:                                        # one more than the table holds: refused, nothing launched
        before = db.host()
        t.n = 65
        assert hip_lib.mmvae_reduce_segments(ctypes.byref(t), H.stream()) == ERR_ARG
        t.n = 0
        assert hip_lib.mmvae_reduce_segments(ctypes.byref(t), H.stream()) == ERR_ARG
        torch.cuda.synchronize()
        assert same_bits(db.host(), before)


def rider_args(H, rng, n_rows, B, n_out):
    stride = B + 3
    rows = np.full(n_rows * stride, 1e6, np.float32)
    rows.reshape(n_rows, stride)[:, :B] = rng.standard_normal((n_rows, B), dtype=np.float32)
    rb = Buf(rows, shift=1)
    rp = H.RowPtrs()
    for i in range(min(n_rows, H.LC_MAX_ROWS)):
        rp.p[i] = rb.ptr + 4 * i * stride
    W = rng.standard_normal((n_out, n_rows)).astype(np.float32)
    wf = (ctypes.c_float * W.size)(*W.ravel().tolist())
    out = Buf(canary_floats(max(n_out, 8))[:n_out])
    return rb, rp, W, wf, out, rows.reshape(n_rows, stride)[:, :B]


def test_reduce_segments_lincomb_rider(hip_lib, H):
    """out_k = sum_n W[k][n] sum_b rows_n[b] as the extra workgroup of a fold launch: the fold is still right, the rider
    is right per output"""
    rng = np.random.default_rng(40)
    specs = [([3], 70, True, True, True), ([130], 9, False, False, False)]
    arena, segs, dst0, ranges = lay_out(rng, specs)
    ab = Buf(arena)
    for n_rows in (1, 5, 32):
        for B in (1, 63, 64, 65, 130):
            for n_out in (1, 4):
                db = Buf(dst0)
                t = table_of(H, segs, ab.ptr, db.ptr)
                rb, rp, W, wf, out, rows = rider_args(H, rng, n_rows, B, n_out)
                rc = hip_lib.mmvae_reduce_segments_lincomb(ctypes.byref(t), ctypes.byref(rp), wf, out.ptr, n_rows, B, n_out,
                                                           H.stream())
                assert rc == 0
                torch.cuda.synchronize()
                assert db.intact() and out.intact() and rb.intact()
                what = f"rider {n_rows} rows x {B}, {n_out} out"
                check_fold(db.host(), dst0, arena, segs, ranges, what)
                ref, bound = R.rider(W, rows)
                within(out.host(), ref, bound, what, None, "rider, fraction of its bound")
    # more rows / outputs than the rider holds: the unsupported code, nothing launched
    db = Buf(dst0)
    t = table_of(H, segs, ab.ptr, db.ptr)
    for n_rows, n_out in ((33, 4), (5, 5)):
        rb, rp, W, wf, out, rows = rider_args(H, rng, n_rows, 8, n_out)
        rc = hip_lib.mmvae_reduce_segments_lincomb(ctypes.byref(t), ctypes.byref(rp), wf, out.ptr, n_rows, 8, n_out, H.stream())
        assert rc == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert same_bits(out.host(), canary_floats(n_out)) and same_bits(db.host(), dst0)


# ---- fold + Adam in one launch -------------------------------------------------------------------------------------------------
GAPS = (0, 1, 2, 3, 4, 5, 2047, 2048, 2049, 4097, 7)


@functools.lru_cache(maxsize=1)
def fold_adam_case():
    """eleven heads: the first at offset 0, the last ending exactly at n; between them gaps that start at every alignment
    mod 4 and sit around the 2048-element plain chunk; wide and narrow heads, chains, unaligned sources and strides"""
    rng = np.random.default_rng(50)
    specs = [([33], 256, True, True, True), ([7], 300, False, True, False), ([130], 77, True, True, True),
             ([5, 130, 33], 64, True, True, True), ([1], 1, False, True, False), ([128], 513, False, True, True),
             ([4, 9], 3, True, True, False), ([127], 255, True, True, True), ([29], 1000, True, True, True),
             ([512], 257, False, True, False), ([9, 2], 13, True, True, True)]
    arena, segs, _, ranges = lay_out(rng, specs, gaps=GAPS)
    n = ranges[-1][1]
    p, g, m, v, x = R.adam_case(n, "mid", seed=7)
    g = g * (rng.random(n) < 0.5).astype(np.float32)          # what the backward kernels wrote straight into g
    gfold, gerr = R.fold(g, arena, segs)
    for a in (arena, p, g, m, v, x, gfold, gerr):
        a.setflags(write=False)
    lo = (ranges[9][0] - 2000) // 4 * 4                      # a range boundary inside the 4097 gap
    assert ranges[8][1] < lo < ranges[9][0] and (ranges[1][0] % 4, ranges[2][0] % 4) != (0, 0)
    return arena, segs, ranges, (p, g, m, v, x), gfold, gerr, lo


def fold_launch(lib, H, bufs, blk, ab, segs, zg, gs, lo=None, hi=None, advance=1, rider=None, order=None):
    n = bufs[0].n
    t = table_of(H, segs, ab.ptr, bufs[1].ptr, order)
    tail = (ctypes.byref(rider[1]), rider[3], rider[4].ptr, *rider[5]) if rider else (None, None, None, 0, 0, 0)
    if lo is None:
        return lib.mmvae_adam_fold_flat(*[b.ptr for b in bufs], n, LR, B1, B2, EPS, blk.ptr, gs, zg, ctypes.byref(t), *tail,
                                        H.stream())
    return lib.mmvae_adam_fold_range(*[b.ptr for b in bufs], n, lo, hi, advance, LR, B1, B2, EPS, blk.ptr, gs, zg,
                                     ctypes.byref(t), *tail, H.stream())


def check_folded_gradient(G, g_before, gfold, gerr, ranges, zg, what, lo=0, hi=None):
    hi = G.size if hi is None else hi
    if zg:
        assert not bits(G[lo:hi]).any(), f"{what}: gradient not cleared"
        return
    m = ~outside(ranges, G.size)
    m[:lo] = False
    m[hi:] = False
    within(G[m], gfold[m], gerr[m], f"{what}: folded gradient", gerr[m] / R.U, "fold, fraction of (R + 1) u sum|terms|")
    assert same_bits(G[~m], g_before[~m]), f"{what}: g changed outside the heads of [{lo}, {hi})"


@pytest.mark.parametrize("zg", [1, 0])
@pytest.mark.parametrize("gs", [0.5, 1.0 / 3.0])
def test_adam_fold_flat_per_element(hip_lib, H, zg, gs):
    """fold + direct gradient, then one Adam step, against float64 for the WHOLE buffer (not against the other spellings
    of the same update); resumed block {41, 0, 0, 0} -> step 42; with the rider"""
    arena, segs, ranges, case, gfold, gerr, _ = fold_adam_case()
    rng = np.random.default_rng(51)
    ab, bufs, blk = Buf(arena, shift=0), [Buf(a) for a in case], Block(41)
    rb, rp, W, wf, out, rows = rider_args(H, rng, 5, 65, 4)
    order = rng.permutation(len(segs)).tolist()
    rc = fold_launch(hip_lib, H, bufs, blk, ab, segs, zg, gs, rider=(rb, rp, W, wf, out, (5, 65, 4)), order=order)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs + [ab, out]), "canaries"
    res = [b.host() for b in bufs]
    what = f"adam_fold_flat zg {zg} gs {gs:.3g}"
    check_adam(case, res, 42, gs, zg, what, g_ref=gfold, g_err=gerr)
    check_folded_gradient(res[1], case[1], gfold, gerr, ranges, zg, what)
    c, tk, r1, r2 = blk.read()
    assert (c, tk) == (42, 0) and abs(r1 / FB1 ** 42 - 1) <= 1e-12 and abs(r2 / FB2 ** 42 - 1) <= 1e-12
    ref, bound = R.rider(W, rows)
    within(out.host(), ref, bound, what + ": rider", None, "rider, fraction of its bound")


@pytest.mark.parametrize("zg", [1, 0])
def test_adam_fold_range_per_element(hip_lib, H, zg):
    """the same step in two launches: [lo, n) without closing the step, then [0, lo) closing it; the full table both times"""
    arena, segs, ranges, case, gfold, gerr, lo = fold_adam_case()
    n = case[0].size
    gs = 1.0 / 3.0
    ab, bufs, blk = Buf(arena), [Buf(a) for a in case], Block(41, FB1 ** 41, FB2 ** 41)
    assert fold_launch(hip_lib, H, bufs, blk, ab, segs, zg, gs, lo=lo, hi=n, advance=0) == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs + [ab]), "canaries"
    mid = [b.host() for b in bufs]
    what = f"adam_fold_range [{lo}, {n}) zg {zg}"
    check_adam(case, mid, 42, gs, zg, what, g_ref=gfold, g_err=gerr, lo=lo, hi=n)      # (bit-untouched outside included)
    check_folded_gradient(mid[1], case[1], gfold, gerr, ranges, zg, what, lo, n)
    assert blk.read() == (41, 0, FB1 ** 41, FB2 ** 41), "advance = 0 must leave the block alone"
    assert fold_launch(hip_lib, H, bufs, blk, ab, segs, zg, gs, lo=0, hi=lo, advance=1) == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs + [ab]), "canaries"
    res = [b.host() for b in bufs]
    for a, b in zip(res, mid):
        assert same_bits(a[lo:], b[lo:]), "the closing launch touched the range already updated"
    what = f"adam_fold_range [0, {lo}) zg {zg}"
    check_adam(case, res, 42, gs, zg, what, g_ref=gfold, g_err=gerr, lo=0, hi=lo, frozen=mid)
    check_folded_gradient(res[1], mid[1], gfold, gerr, ranges, zg, what, 0, lo)
    c, tk, r1, r2 = blk.read()
    assert (c, tk) == (42, 0) and abs(r1 / FB1 ** 42 - 1) <= 1e-12


def test_adam_fold_refusals_launch_nothing(hip_lib, H):
    arena, segs, ranges, case, gfold, gerr, lo = fold_adam_case()
    n = case[0].size
    ab, bufs, blk = Buf(arena), [Buf(a) for a in case], Block(41)
    rng_launch = lambda sg, lo_, hi_: fold_launch(hip_lib, H, bufs, blk, ab, sg, 1, 1.0, lo=lo_, hi=hi_, advance=1)
    assert rng_launch(segs, lo + 2, n) == ERR_ARG                 # lo % 4 != 0
    assert rng_launch(segs, lo, lo) == ERR_ARG                    # lo >= hi
    assert rng_launch(segs, n, lo) == ERR_ARG
    assert rng_launch(segs, lo, n + 4) == ERR_ARG                 # hi > n
    inside = ranges[9][0]
    assert rng_launch([(0, inside, 32768, 16, 16)], lo, n) == ERR_ARG                 # rows do not fit the table's short
    assert rng_launch([(0, ranges[8][1] - 8, 2, lo - ranges[8][1] + 16, 4200)], lo, n) == ERR_ARG   # straddles lo
    # a destination outside the flat buffer is nobody's segment: refused by EVERY range launch, not skipped as "another
    # launch's" (behind the end, in front of the start, straddling the end), and by the whole-buffer form
    for sg in ((0, n, 2, 16, 16), (0, -16, 2, 16, 16), (0, n - 8, 2, 16, 16), (0, n + 4096, 2, 16, 16)):
        assert rng_launch([sg], 0, lo) == ERR_ARG, sg
        assert rng_launch([sg], lo, n) == ERR_ARG, sg
        assert rng_launch([segs[0], sg], 0, lo) == ERR_ARG, sg
        assert fold_launch(hip_lib, H, bufs, blk, ab, [sg], 1, 1.0) == ERR_ARG, sg
    # overlapping destination ranges would race
    assert fold_launch(hip_lib, H, bufs, blk, ab, [(0, 100, 2, 16, 16), (64, 108, 2, 16, 16)], 1, 1.0) == ERR_ARG
    for k in range(5):
        ptrs = [b.ptr for b in bufs]
        ptrs[k] += 4
        t = table_of(H, segs, ab.ptr, bufs[1].ptr)
        assert hip_lib.mmvae_adam_fold_flat(*ptrs, n - 4, LR, B1, B2, EPS, blk.ptr, 1.0, 1, ctypes.byref(t), None, None, None,
                                            0, 0, 0, H.stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert all(b.intact() and same_bits(b.host(), a) for b, a in zip(bufs, case)) and blk.read() == (41, 0, 0.0, 0.0)


def test_adam_fold_range_without_segments_is_plain_adam(hip_lib, H):
    """no table at all, and a table whose segments all belong to the other range"""
    arena, segs, ranges, case, gfold, gerr, lo = fold_adam_case()
    n = case[0].size
    ab = Buf(arena)
    for table in (None, [s for s in segs if s[1] < lo]):
        bufs, blk = [Buf(a) for a in case], Block(41)
        if table is None:
            rc = hip_lib.mmvae_adam_fold_range(*[b.ptr for b in bufs], n, lo, n, 0, LR, B1, B2, EPS, blk.ptr, 1.0, 0, None,
                                               None, None, None, 0, 0, 0, H.stream())
        else:
            rc = fold_launch(hip_lib, H, bufs, blk, ab, table, 0, 1.0, lo=lo, hi=n, advance=0)
        assert rc == 0
        torch.cuda.synchronize()
        assert all(b.intact() for b in bufs)
        check_adam(case, [b.host() for b in bufs], 42, 1.0, 0, "plain range", lo=lo, hi=n)


# ---- fill, step_inc ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 524293])
def test_fill(hip_lib, H, n):
    for shift, value in ((0, 0.0), (1, -1.5), (3, 3.0e38)):
        b = Buf(np.full(n, np.nan, np.float32), shift=shift)
        assert hip_lib.mmvae_fill(b.ptr, n, value, H.stream()) == 0
        torch.cuda.synchronize()
        assert b.intact() and same_bits(b.host(), np.full(n, value, np.float32))
    assert hip_lib.mmvae_fill(b.ptr, 0, 1.0, H.stream()) == ERR_ARG and hip_lib.mmvae_fill(None, 4, 1.0, H.stream()) == ERR_ARG


def test_step_inc(hip_lib, H):
    blk = Block(41, 0.25, 0.5)
    for _ in range(3):
        assert hip_lib.mmvae_step_inc(blk.ptr, H.stream()) == 0
    torch.cuda.synchronize()
    assert blk.read() == (44, 0, 0.25, 0.5)
    assert hip_lib.mmvae_step_inc(None, H.stream()) == ERR_ARG
