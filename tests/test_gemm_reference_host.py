"""CPU checks of tests/gemm_reference.py, the yardstick of tests/test_gemm_gpu.py: the float64 restatement equals torch,
the path names are the header's, the case table reaches the kernels it names (asked of the library's own selectors, which
launch nothing), the split mirrors that size workspaces agree with the dispatcher over a grid of shapes, the memory-layout
plumbing passes an exact result and sees a stray write, and the part-by-part checker catches seeded errors on exactly the
part that carries them."""
import ctypes
import itertools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import gemm_reference as GR

F64 = torch.float64


def _lib():
    from multimodal_vae_comparison_amd import hipops
    return hipops.lib()


def _close(a, b, what, tol=1e-12):
    e = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    assert e <= tol, f"{what}: {e:.3e}"


_TORCH_ACT = {GR.ACT_NONE: lambda t: t, GR.ACT_SILU: F.silu, GR.ACT_RELU: torch.relu, GR.ACT_GELU: F.gelu}


# ---------------------------------------------------------------------------------------------
# the restatement equals torch in float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [GR.ACT_NONE, GR.ACT_SILU, GR.ACT_RELU, GR.ACT_GELU])
@pytest.mark.parametrize("M,N,K", [(5, 7, 9), (1, 1, 1), (33, 2, 17)])
def test_linear_reference_equals_torch_and_autograd(M, N, K, act):
    g = torch.Generator().manual_seed(100 * M + 10 * N + K + act)
    x, w, b, dy = (torch.randn(*s, generator=g, dtype=F64) for s in ((M, K), (N, K), (N,), (M, N)))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.linear(_TORCH_ACT[act](xr), wr, br)
    y.backward(dy)
    _close(GR.linear_fwd_reference(x, w, b, None, act)["y"], y.detach(), "y")
    ep = {GR.ACT_NONE: GR.EP_NONE, GR.ACT_SILU: GR.EP_MUL_SILU_GRAD, GR.ACT_RELU: GR.EP_MUL_RELU_MASK,
          GR.ACT_GELU: GR.EP_MUL_GELU_GRAD}[act]
    r = GR.linear_bwd_reference(dy, x, w, x if ep else None, x_act=act, ep=ep)
    for part, t in (("dx", xr), ("dw", wr), ("db", br)):
        _close(r[part], t.grad, part)
    # the wrappers alone, accumulating into old contents
    old_w, old_b, old_x = torch.randn(N, K, generator=g, dtype=F64), torch.randn(N, generator=g, dtype=F64), torch.randn(M, K, generator=g, dtype=F64)
    r = GR.linear_bwd_weight_reference(dy, x, old_w, old_b, act, 1)
    _close(r["dw"], wr.grad + old_w, "dw accumulated")
    _close(r["db"], br.grad + old_b, "db accumulated")
    _close(GR.linear_bwd_data_reference(dy, w, x if ep else None, old_x, ep, 1)["dx"], xr.grad + old_x, "dx accumulated")


def test_gemm_reference_equals_conv_transpose_on_a_1x1_input():
    """the weight layout of ops.LinearKN: (K, C, kh, kw), the reduction index outermost"""
    g = torch.Generator().manual_seed(3)
    M, K, C, kh, kw = 6, 5, 3, 2, 4
    x, w = torch.randn(M, K, generator=g, dtype=F64), torch.randn(K, C, kh, kw, generator=g, dtype=F64)
    dy = torch.randn(M, C * kh * kw, generator=g, dtype=F64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv_transpose2d(F.silu(xr).view(M, K, 1, 1), wr).reshape(M, -1)
    y.backward(dy)
    w2 = w.view(K, -1)
    _close(GR.gemm_reference(x, w2, a_act=GR.ACT_SILU)["C"], y.detach(), "y")
    _close(GR.gemm_reference(dy, w2.t(), None, x, ep=GR.EP_MUL_SILU_GRAD)["C"], xr.grad, "dx")
    _close(GR.gemm_reference(x.t(), dy, a_act=GR.ACT_SILU)["C"], wr.grad.view(K, -1), "dw")


def test_epilogues_equal_torch():
    g = torch.Generator().manual_seed(4)
    v = torch.randn(200, generator=g, dtype=F64) * 4
    aux = torch.randn(200, generator=g, dtype=F64) * 3
    aux[:4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=F64)
    E = GR.epilogue
    _close(E(v, None, GR.EP_RELU), torch.relu(v), "relu")
    _close(E(v, None, GR.EP_GELU), F.gelu(v), "gelu")
    _close(E(v, None, GR.EP_SIGMOID), torch.sigmoid(v), "sigmoid")
    lo, hi = torch.tensor(1e-6, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-6, dtype=torch.float32)
    _close(E(v * 5, None, GR.EP_SIGMOID_CLAMP), torch.sigmoid(v * 5).clamp(float(lo), float(hi)), "sigmoid clamp")
    assert float(E(v * 50, None, GR.EP_SIGMOID_CLAMP).min()) == float(lo) and float(E(v * 50, None, GR.EP_SIGMOID_CLAMP).max()) == float(hi)
    _close(E(v, aux, GR.EP_ADD_AUX), v + aux, "add aux")
    mask = E(v, aux, GR.EP_MUL_RELU_MASK)
    _close(mask, v * (aux > 0), "relu mask")
    assert float(mask[0]) == 0.0 and float(mask[1]) == 0.0 and float(mask[2]) == float(v[2]) and float(mask[3]) == 0.0
    for ep, fn in ((GR.EP_MUL_SILU_GRAD, F.silu), (GR.EP_MUL_GELU_GRAD, F.gelu)):
        a = aux.clone().requires_grad_(True)
        fn(a).backward(v)
        _close(E(v, aux, ep), a.grad, f"epilogue {ep}")
    for act in (GR.ACT_SILU, GR.ACT_RELU, GR.ACT_GELU):
        _close(GR.act(v, act), _TORCH_ACT[act](v), f"act {act}")


def test_row_sums_splits_and_the_aux_write():
    g = torch.Generator().manual_seed(5)
    M, N, K, kper = 7, 5, 23, 8
    A, B, bias = (torch.randn(*s, generator=g, dtype=F64) for s in ((M, K), (K, N), (N,)))
    old, rs_old = torch.randn(M, N, generator=g, dtype=F64), torch.randn(M, generator=g, dtype=F64)
    r = GR.gemm_reference(A, B, bias, A[:0], ep=GR.EP_GELU, a_act=GR.ACT_SILU, rowsum=True)
    _close(r["aux"], F.silu(A) @ B + bias, "aux receives the pre-activation")
    _close(r["C"], F.gelu(F.silu(A) @ B + bias), "C")
    _close(r["rowsum"], F.silu(A).sum(1), "row sums of act(A)")
    assert "aux" not in GR.gemm_reference(A, B, bias, None, ep=GR.EP_GELU)
    p = GR.gemm_reference(A, B, None, None, old, rs_old, accumulate=GR.ACC_DEFER, rowsum=True, nz=3, kper=kper)
    assert set(p) == {"partial", "rs_partial"} and p["partial"].shape == (3, M, N) and p["rs_partial"].shape == (3, M)
    _close(p["partial"][2], A[:, 16:] @ B[16:], "the short last split")
    _close(p["partial"].sum(0), A @ B, "partials sum to the product")
    _close(p["rs_partial"].sum(0), A.sum(1), "row-sum partials")
    one = GR.gemm_reference(A, B, None, None, old, rs_old, accumulate=GR.ACC_DEFER, rowsum=True, nz=1, kper=K)
    _close(one["C"], A @ B + old, "DEFER with one split is a plain accumulate")
    _close(one["rowsum"], A.sum(1) + rs_old, "... of the row sums too")
    s = GR.strided(torch.arange(40, dtype=F64), 3, 4, 5, 1, 6)
    assert float(s[2, 3]) == 3 + 2 + 18


def test_reference_passes_gradcheck():
    g = torch.Generator().manual_seed(6)
    x, w, b = (torch.randn(*s, generator=g, dtype=F64).requires_grad_(True) for s in ((3, 4), (2, 4), (2,)))
    f = lambda x_, w_, b_: GR.linear_fwd_reference(x_, w_, b_, None, GR.ACT_SILU, GR.EP_GELU)["y"]
    assert torch.autograd.gradcheck(f, (x, w, b))


# ---------------------------------------------------------------------------------------------
# the case table and the library's selectors
# ---------------------------------------------------------------------------------------------
def test_path_names_match_the_header():
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    body = re.search(r"enum \{\s*MMVAE_GEMM_B16_KK_1 = (\d+),(.*?)\};", src, flags=re.S)
    names = ["B16_KK_1"] + re.findall(r"MMVAE_GEMM_(\w+)", body.group(2))
    assert tuple(names) == GR.PATHS and int(body.group(1)) == GR.PATH_VALUE["B16_KK_1"]


def _family(path):
    return re.sub(r"_(KK|KN|MK|MN|VV|VS|SV|SS)(?=_|$)", "", path)


# families whose reduction a call can split over workgroups
_SPLITTING = {"STAGED1", "STAGED4", "BIG128", "BIG64", "RSPLIT_16", "RSPLIT_64", "LINBWD_B16_1", "LINBWD_B16_2", "LINBWD_STAGED"}


def _gemm_dims(c, nz, kper):
    """(rows, cols, reduction) of the problems of a case: what can be ragged against a tile"""
    M, N, K = c.M, c.N, c.K
    return {"gemm": [(M, N, K)], "linear_fwd": [(M, N, K)], "bwd_data": [(M, K, N)], "bwd_weight": [(N, K, M)],
            "linear_bwd": [(M, K, N), (N, K, M)]}[c.entry]


def test_case_table_reaches_the_kernels_it_names():
    """every case, asked of the library's own selector with the split-bf16 core on and off; the union is every
    instantiation but UNREACHABLE; every family is reached from a ragged M, N and K and, where it can split, from a
    split reduction whose last split is short"""
    lib = _lib()
    assert len({c.name for c in GR.CASES}) == len(GR.CASES)
    seen = {}
    was = lib.mmvae_gemm_b16_set(1)
    try:
        for c in GR.CASES:
            for core, want in ((1, c.path), (0, c.path0)):
                lib.mmvae_gemm_b16_set(core)
                p, nz, kper = c.query(lib)
                assert GR.PATH_NAME.get(p, p) == want, f"{c} (split-bf16 {core}): selector gives {GR.PATH_NAME.get(p, p)}, the case names {want}"
                s = seen.setdefault(_family(want), {"paths": set(), "ragged": set(), "short": False})
                s["paths"].add(want)
                for rows, cols, red in _gemm_dims(c, nz, kper):
                    s["ragged"] |= {n for n, v in (("M", rows), ("N", cols), ("K", red)) if v % 16}
                if nz > 1:
                    red = c.reductions()[-1]
                    assert (nz - 1) * kper < red <= nz * kper
                    s["short"] |= red % kper != 0
    finally:
        lib.mmvae_gemm_b16_set(was)
    reached = set().union(*(s["paths"] for s in seen.values()))
    assert reached == set(GR.PATHS) - set(GR.UNREACHABLE), sorted(reached ^ (set(GR.PATHS) - set(GR.UNREACHABLE)))
    for fam, s in seen.items():
        need = {"M"} if fam == "PROJ32" else {"M", "N", "K"}      # PROJ32: K = 32 and N % 32 == 0 are the kernel's shape
        assert need <= s["ragged"], f"{fam}: no case ragged in {sorted(need - s['ragged'])}"
        assert s["short"] or fam not in _SPLITTING, f"{fam}: no case with a short last split"


GRID = (1, 3, 31, 32, 33, 127, 128, 129, 383, 384, 1024, 1025, 2047, 2048, 4096, 4097)


def test_split_mirrors_agree_with_the_dispatcher():
    """mmvae_linear_bwd_weight_splits, mmvae_linear_bwd_splits and mmvae_gemm_splits size ops.py's GradReducer partial
    counts, the *_ws_floats its workspaces: over the grid they equal the nz the path queries report and hold nz partials"""
    lib = _lib()
    nz, kper = ctypes.c_int(0), ctypes.c_int(0)
    out = (ctypes.byref(nz), ctypes.byref(kper))
    was = lib.mmvae_gemm_b16_set(1)
    try:
        for core in (1, 0):
            lib.mmvae_gemm_b16_set(core)
            for M, N, K in itertools.product(GRID, GRID, GRID):
                for has_db in (1, 0):
                    p = lib.mmvae_linear_bwd_weight_path(M, N, K, K, 0, 0, has_db, 1, 1, *out)
                    assert p > 0 and nz.value == lib.mmvae_linear_bwd_weight_splits(M, N, K), (core, M, N, K, has_db, p, nz.value)
                    assert nz.value == 1 or lib.mmvae_linear_bwd_weight_ws_floats(M, N, K) >= nz.value * (N * K + N), (core, M, N, K)
                    p = lib.mmvae_linear_bwd_path(M, N, K, K, 0, 0, 0, has_db, 1, 1, 1, *out)
                    if p > 0:      # (-ERR_ARG: a split-bf16 shape whose ldx = K is no multiple of 4 cannot occur: K % 4 == 0 there)
                        assert nz.value == lib.mmvae_linear_bwd_splits(M, N, K), (core, M, N, K, has_db, p, nz.value)
                        assert nz.value == 1 or lib.mmvae_linear_bwd_ws_floats(M, N, K) >= nz.value * (N * K + N), (core, M, N, K)
                    else:
                        assert False, (core, M, N, K, p)
                for splitk in (1, 2, 7, 64):
                    for sam, sak, sbk, sbn in ((K, 1, 1, K), (1, M, N, 1)):
                        p = lib.mmvae_gemm_path(M, N, K, sam, sak, sbk, sbn, N, 0, 0, 0, 0, splitk, 0, 1, 1, *out)
                        if p < 0:      # K = 1 or M = 1 make both strides of an operand 1; the m-major form of M = 1 reads as k-major
                            assert p == -GR.ERR_UNSUPPORTED, (M, N, K, p)
                            continue
                        assert nz.value == lib.mmvae_gemm_splits(M, N, K, splitk), (core, M, N, K, splitk, p, nz.value)
                        assert nz.value <= splitk and (nz.value - 1) * kper.value < K <= nz.value * kper.value
                        assert nz.value == 1 or lib.mmvae_gemm_ws_floats(M, N, splitk) >= nz.value * (M * N + M)
    finally:
        lib.mmvae_gemm_b16_set(was)


def test_selectors_refuse_what_the_launchers_refuse():
    lib = _lib()
    q = lib.mmvae_gemm_path
    assert q(0, 4, 4, 4, 1, 1, 4, 4, 0, 0, 0, 0, 1, 0, 1, 1, None, None) == -GR.ERR_ARG
    assert q(4, 4, 4, 8, 2, 1, 4, 4, 0, 0, 0, 0, 1, 0, 1, 1, None, None) == -GR.ERR_UNSUPPORTED      # A: neither stride is 1
    assert q(4, 4, 4, 4, 1, 2, 8, 4, 0, 0, 0, 0, 1, 0, 1, 1, None, None) == -GR.ERR_UNSUPPORTED      # B likewise
    # splits that the call sums itself are written as M * N contiguous floats: ldc must be N (deferred partials: any ldc)
    split = lambda ldc, acc: q(33, 17, 300, 300, 1, 17, 1, ldc, 0, 0, 0, acc, 3, 0, 1, 1, None, None)
    assert split(20, 0) == split(20, 1) == -GR.ERR_UNSUPPORTED
    assert split(17, 0) == split(17, 1) == split(20, GR.ACC_DEFER) == GR.PATH_VALUE["STAGED4_KN"]
    assert lib.mmvae_linear_bwd_path(0, 4, 4, 4, 0, 0, 0, 1, 1, 1, 1, None, None) == -GR.ERR_ARG
    assert lib.mmvae_linear_bwd_path(8, 4, 4, 4, 0, 0, 0, 1, 0, 1, 1, None, None) == -GR.ERR_ARG     # register form: dy off 16 bytes
    was = lib.mmvae_gemm_b16_set(1)
    try:
        assert lib.mmvae_linear_bwd_path(2048, 128, 128, 129, 0, 0, 0, 1, 1, 1, 1, None, None) == -GR.ERR_ARG      # ldx % 4
        assert lib.mmvae_linear_bwd_path(2048, 128, 128, 128, 0, 0, 0, 1, 1, 1, 0, None, None) == -GR.ERR_ARG      # W off 16 bytes
    finally:
        lib.mmvae_gemm_b16_set(was)


# ---------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------
def _case(path, **attrs):
    hits = [c for c in GR.CASES if c.path == path and all(getattr(c, k) == v for k, v in attrs.items())]
    assert hits, (path, attrs)
    return hits[0]


def _exact(case, nz=1, kper=None):
    inp = GR.make_inputs(case)
    ref, bounds = GR.expected(case, inp, nz, kper)
    return inp, ref, bounds, {p: t.float() for p, t in ref.items()}


def _failing(case, got, ref, bounds):
    return {p for p, (ok, _, _, _) in GR.check_parts(case, got, ref, bounds).items() if not ok}


def test_the_exact_result_passes_through_the_layout_and_a_stray_write_shows():
    """the float32 rounding of the reference, written through build_buffers / read back by collect, passes every part of
    every small case; one float changed in a padding column, past the last row, in an input or past the partials is seen"""
    lib = _lib()
    small = [c for c in GR.CASES if c.M * c.N * max(c.reductions()) <= 2_000_000]
    assert len(small) >= 40
    for c in small:
        p, nz, kper = c.query(lib)
        inp, ref, bounds, exact = _exact(c, nz, kper)
        rows, cols = GR.split_dims(c)
        bufs = GR.build_buffers(c, inp, nz * (rows * cols + rows) + 5)
        for part, t in exact.items():
            if part.endswith("partial"):
                ws = bufs["ws"].view().reshape(-1)
                first = 0 if part in ("partial", "dw_partial") else nz * rows * cols
                ws[first: first + t.numel()] = t.reshape(-1)
            else:
                name = {"C": "C", "y": "y", "aux": "aux"}.get(part, part)
                bufs[name].view().copy_(t.reshape(bufs[name].rows, bufs[name].cols))
        got = GR.collect(c, bufs, nz)
        assert not _failing(c, got, ref, bounds), c
        assert GR.memory_violations(c, bufs, nz) == [], c
        main = [n for n in ("C", "y", "dx", "dw") if n in bufs][0]
        spots = {main: [GR.GUARD + bufs[main].off + bufs[main].rows * bufs[main].ld, GR.GUARD - 1],
                 [n for n in ("A", "x", "dy") if n in bufs][0]: [GR.GUARD + 2]}
        if bufs[main].ld > bufs[main].cols:
            spots[main].append(GR.GUARD + bufs[main].off + bufs[main].cols)
        if "ws" in bufs:
            spots["ws"] = [GR.GUARD + (nz * (rows * cols + rows) if nz > 1 else 0)]
        for name, idx in spots.items():
            for i in idx:
                keep = bufs[name].flat[i].clone()
                bufs[name].flat[i] = 1.0
                assert any(m.startswith(name + ":") for m in GR.memory_violations(c, bufs, nz)), (c, name, i)
                bufs[name].flat[i] = keep
        assert GR.memory_violations(c, bufs, nz) == [], c


def test_checker_catches_seeded_errors_on_the_part_that_carries_them():
    """each error a kernel of this kind can have, applied to the float64 result of a table case and rounded to float32:
    the checker fails on exactly the named part.  This, not a number, shows the tolerances are tight enough."""
    lib = _lib()
    d64 = lambda inp: {k: v.to(F64) for k, v in inp.items()}

    # the last k-slice of a ragged K dropped
    c = _case("R16_16_SS", K=21, ep=GR.EP_MUL_SILU_GRAD)
    inp, ref, bounds, got = _exact(c)
    short = dict(inp, A=inp["A"][:, :-1].contiguous(), B=inp["B"][:-1].contiguous())
    got["C"] = GR.expected(c, short)[0]["C"].float()
    assert _failing(c, got, ref, bounds) == {"C"}

    # the last row of an edge tile left at its old value
    c = _case("R16_16_SS", acc=1, pad_a=1)
    inp, ref, bounds, got = _exact(c)
    got["C"][-1] = inp["c_old"][-1]
    assert _failing(c, got, ref, bounds) == {"C"}

    # the bias shifted by one column
    c = _case("R32_16_VV", rowsum=True, bias=True)
    inp, ref, bounds, got = _exact(c)
    got["C"] = GR.expected(c, dict(inp, bias=inp["bias"].roll(1)))[0]["C"].float()
    assert _failing(c, got, ref, bounds) == {"C"}

    # one split partial missing
    c = _case("RSPLIT_16", entry="gemm", acc=GR.ACC_DEFER)
    _, nz, kper = c.query(lib)
    assert nz == 3
    inp, ref, bounds, got = _exact(c, nz, kper)
    assert set(ref) == {"partial", "rs_partial"}
    got["partial"][1] = 0.0
    assert _failing(c, got, ref, bounds) == {"partial"}

    # the row sum taken of A instead of act(A)
    c = _case("R32_16_SV", rowsum=True, a_act=GR.ACT_SILU)
    inp, ref, bounds, got = _exact(c)
    got["rowsum"] = d64(inp)["A"].sum(1).float()
    assert _failing(c, got, ref, bounds) == {"rowsum"}

    # the ReLU mask taken as aux >= 0 (the table's aux holds 0 and -0)
    c = _case("R16_16_SS", orient="MN", ep=GR.EP_MUL_RELU_MASK)
    inp, ref, bounds, got = _exact(c)
    aux = d64(inp)["aux"]
    assert int((aux == 0).sum()) >= 2
    v = d64(inp)["A"] @ d64(inp)["B"]
    got["C"] = torch.where(aux >= 0, v, torch.zeros_like(v)).float()
    assert _failing(c, got, ref, bounds) == {"C"}

    # EP_GELU's aux receiving the activated value
    c = _case("R16_16_VS", orient="KN", ep=GR.EP_GELU)
    inp, ref, bounds, got = _exact(c)
    got["aux"] = got["C"].clone()
    assert _failing(c, got, ref, bounds) == {"aux"}


def test_checker_sees_what_the_max_norm_cannot():
    """a small-magnitude element wrong by many ulps passes the max-norm tolerance and fails its own bound"""
    c = _case("R16_16_VV", bias=True, ep=GR.EP_RELU)
    inp, ref, bounds, got = _exact(c)
    i = int(bounds["C"].argmin())      # an element whose operands are all small
    got["C"].view(-1)[i] += 0.1 * GR.CAP_FP32["out"] * float(ref["C"].abs().max())      # a tenth of the max-norm tolerance
    res = GR.check_parts(c, got, ref, bounds)["C"]
    assert not res[0] and res[1] < 1.0 < res[2], res


def test_function_error_table():
    """e_fn: E_FN_MARGIN x the float32 torch-CPU error of each elementwise function on the table's own inputs (never
    below the floor the number format gives).  Printed per function (DESIGN.md holds the table); the figures are those of
    float32 arithmetic: a few U of the function's value or argument"""
    worst = {}
    for c in GR.CASES:
        if c.M * c.N * max(c.reductions()) > 2_000_000:
            continue
        inp = GR.make_inputs(c)
        ops_ = [(f"act {a}", GR.act_err(t, a)) for a, t in ((c.a_act, inp.get("A", inp.get("x"))), (c.b_act, inp.get("B")))
                if a in (GR.ACT_SILU, GR.ACT_GELU) and t is not None]
        if c.ep not in (GR.EP_NONE, GR.EP_RELU, GR.EP_MUL_RELU_MASK, GR.EP_ADD_AUX) and c.entry == "gemm":
            v = GR.gemm_reference(inp["A"].double(), inp["B"].double(), a_act=c.a_act, b_act=c.b_act)["C"]
            aux = inp.get("aux")
            ops_.append((f"ep {c.ep}", GR.ep_fn_err(v, aux, c.ep) / (v.abs().clamp_min(1.0) if c.ep in (GR.EP_MUL_SILU_GRAD, GR.EP_MUL_GELU_GRAD) else 1.0)))
        for name, e in ops_:
            worst[name] = max(worst.get(name, 0.0), float(e.max()))
            print(f"e_fn {c.name} {name}: {float(e.max()):.3e}")
    for name, e in sorted(worst.items()):
        print(f"e_fn worst {name}: {e:.3e} = {e / GR.U:.1f} U")
        assert 0.0 < e <= 64 * 20 * GR.U, (name, e)      # arguments up to 20: a handful of U of the argument
    assert {"act 1", "act 3", "ep 3", "ep 4", "ep 5", "ep 6", "ep 7"} <= set(worst), sorted(worst)
