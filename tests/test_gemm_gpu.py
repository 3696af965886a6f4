"""The GEMM core (csrc/gemm.hip, gemm_b16.inc) on the GPU against tests/gemm_reference.py: every case of its table
through its real entry point -- mmvae_gemm_f32, mmvae_linear_fwd, mmvae_linear_bwd_data, mmvae_linear_bwd_weight,
mmvae_linear_bwd by ctypes, ops.linear / ops.LinearKN through autograd.  Per case: the library names the kernel the case is
for (asked with the actual pointers, before the launch); every part (C, row sums, the aux write, each deferred partial,
dx, dW, db) is held to the suite's max-norm tolerance AND to the per-element bound of gemm_reference.gemm_bounds; and
every float the call may not write -- padding columns, rows past the end, guard bands, inputs, ws past the partials, a
deferred destination -- is bit-identical afterwards.  Cases the split-bf16 core takes run with it on and off."""
import ctypes

import pytest
import torch

import gemm_reference as GR

pytestmark = pytest.mark.gpu
DEV = "cuda"
_INPUTS = {}


def _inputs(case):
    if case.name not in _INPUTS:
        _INPUTS.clear()      # one case's inputs at a time (the largest are tens of MB)
        _INPUTS[case.name] = GR.make_inputs(case)
    return _INPUTS[case.name]


def _ws_floats(lib, c):
    if c.entry == "gemm":
        return lib.mmvae_gemm_ws_floats(c.M, c.N, c.splitk)
    if c.entry == "bwd_weight":
        return lib.mmvae_linear_bwd_weight_ws_floats(c.M, c.N, c.K)
    if c.entry == "linear_bwd":
        return lib.mmvae_linear_bwd_ws_floats(c.M, c.N, c.K)
    return 0


def _p(bufs, name):
    return ctypes.c_void_p(bufs[name].ptr) if name in bufs else None


def _launch(lib, c, b):
    from multimodal_vae_comparison_amd import hipops as H
    st, M, N, K = H.stream(), c.M, c.N, c.K
    if c.entry == "gemm":
        return lib.mmvae_gemm_f32(_p(b, "A"), _p(b, "B"), _p(b, "bias"), _p(b, "aux"), _p(b, "C"), _p(b, "rowsum"), _p(b, "ws"),
                                  M, N, K, *c.strides(), c.a_act, c.b_act, c.ep, c.acc, c.splitk, st)
    if c.entry == "linear_fwd":
        return lib.mmvae_linear_fwd(_p(b, "x"), _p(b, "w"), _p(b, "bias"), _p(b, "aux"), _p(b, "y"), M, N, K, c.ldx, c.a_act,
                                    c.ep, st)
    if c.entry == "bwd_data":
        return lib.mmvae_linear_bwd_data(_p(b, "dy"), _p(b, "w"), _p(b, "aux"), _p(b, "dx"), M, N, K, c.ep, c.acc, st)
    if c.entry == "bwd_weight":
        return lib.mmvae_linear_bwd_weight(_p(b, "dy"), _p(b, "x"), _p(b, "dw"), _p(b, "db"), _p(b, "ws"), M, N, K, c.ldx,
                                           c.a_act, c.acc, st)
    return lib.mmvae_linear_bwd(_p(b, "dy"), _p(b, "x"), _p(b, "w"), _p(b, "aux"), _p(b, "dx"), _p(b, "dw"), _p(b, "db"),
                                _p(b, "ws"), M, N, K, c.ldx, c.a_act, c.ep, c.acc, st)


_FIRST = {"gemm": ("A", "B", "C"), "linear_fwd": ("x", "w", "y"), "bwd_data": ("dy", "w", "dx"),
          "bwd_weight": ("dy", "x", "dw"), "linear_bwd": ("dy", "x", "w")}


def _report(case, core, path, res):
    for part, (ok, r_max, r_el, _) in sorted(res.items()):
        print(f"GEMM_RATIO {path} {case.name} b16={core} {part} max-norm {r_max:.3f} per-element {r_el:.3f}")


def _run(lib, case, core):
    want = case.path if core else case.path0
    inp = _inputs(case)
    ws_floats = _ws_floats(lib, case)
    bufs = GR.build_buffers(case, inp, ws_floats, DEV)
    a, b_, c_ = (bufs[n] for n in _FIRST[case.entry])
    al_c = c_.aligned16 and ("bias" not in bufs or bufs["bias"].aligned16)
    path, nz, kper = case.query(lib, a.aligned16, b_.aligned16, al_c)
    assert GR.PATH_NAME.get(path, path) == want, f"{case}: the library names {GR.PATH_NAME.get(path, path)}, the case is for {want}"
    rows, cols = GR.split_dims(case)
    assert nz == 1 or ws_floats >= nz * (rows * cols + rows), f"{case}: {ws_floats} floats of ws for {nz} partials"
    rc = _launch(lib, case, bufs)
    torch.cuda.synchronize()
    assert rc == 0, f"{case}: return code {rc}"
    b16 = want.startswith("B16") or want.startswith("LINBWD_B16")
    ref, bounds = GR.expected(case, inp, nz, kper, b16)
    got = GR.collect(case, bufs, nz)
    res = GR.check_parts(case, got, ref, bounds, b16)
    if GR.deferred(case, nz):      # the partials, reduced in float64, are the product
        for p in [k for k in ref if k.endswith("partial")]:
            cap = (GR.CAP_B16 if b16 else GR.CAP_FP32)[GR.gemm_part_kind(case, p)]
            res[p + "-sum"] = GR.check_part(p + "-sum", got[p].double().sum(0), ref[p].sum(0), bounds[p].sum(0), cap)
    _report(case, core, want, res)
    bad = [m for ok, _, _, m in res.values() if not ok] + GR.memory_violations(case, bufs, nz)
    assert not bad, f"{case} (split-bf16 core {'on' if core else 'off'}, {want}, nz {nz}, kper {kper}):\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("case", GR.CASES, ids=lambda c: c.name)
def test_gemm_case(hip_lib, case):
    was = hip_lib.mmvae_gemm_b16_set(1)
    try:
        for core in ((1, 0) if case.path != case.path0 else (1,)):
            hip_lib.mmvae_gemm_b16_set(core)
            _run(hip_lib, case, core)
    finally:
        hip_lib.mmvae_gemm_b16_set(was)


def test_self_reduced_split_with_padded_ldc_is_refused(hip_lib):
    """found by this table: with nz > 1 and accumulate != DEFER the call sums its partials through mmvae_reduce_rows, which
    writes C as M * N contiguous floats -- with ldc = N + 3 the result landed in the padding columns and the matrix's tail
    stayed unwritten.  Such a call is refused now (the selector says so) and nothing is written."""
    case = GR.Case("gemm", 33, 17, 300, "STAGED4_KN", orient="KN", splitk=3, ldc_pad=3)
    bufs = GR.build_buffers(case, GR.make_inputs(case), hip_lib.mmvae_gemm_ws_floats(33, 17, 3), DEV)
    assert case.query(hip_lib, bufs["A"].aligned16, bufs["B"].aligned16)[0] == -GR.ERR_UNSUPPORTED
    assert _launch(hip_lib, case, bufs) == GR.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values())


# ---------------------------------------------------------------------------------------------
# the autograd plumbing above the same entry points
# ---------------------------------------------------------------------------------------------
_DACT = {GR.ACT_NONE: GR.EP_NONE, GR.ACT_SILU: GR.EP_MUL_SILU_GRAD, GR.ACT_RELU: GR.EP_MUL_RELU_MASK, GR.ACT_GELU: GR.EP_MUL_GELU_GRAD}


def _check(case_like, got, ref, bounds):
    res = {p: GR.check_part(p, got[p].detach().cpu(), ref[p], bounds[p], GR.CAP_FP32["out" if p == "y" else "db" if p == "db" else "grad"])
           for p in ref}
    for p, (ok, r_max, r_el, _) in sorted(res.items()):
        print(f"GEMM_RATIO ops {case_like} {p} max-norm {r_max:.3f} per-element {r_el:.3f}")
    bad = [m for ok, _, _, m in res.values() if not ok]
    assert not bad, f"{case_like}:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("M,N,K,act,fwd,bwd", [(17, 20, 33, GR.ACT_SILU, "R16_16_SS", "LINBWD_R_16_T16"),
                                               (33, 5, 20, GR.ACT_RELU, "R16_16_VV", "LINBWD_STAGED"),
                                               (353, 388, 356, GR.ACT_GELU, "R32_16_VV", "LINBWD_R_64_T32")])
def test_ops_linear_autograd(hip_lib, M, N, K, act, fwd, bwd):
    """ops.linear: mmvae_linear_fwd, then mmvae_linear_bwd with the activation's derivative as the data gradient's epilogue"""
    from multimodal_vae_comparison_amd import ops
    c = GR.Case("linear_bwd", M, N, K, bwd, rowsum=True, a_act=act, ep=_DACT[act])
    inp = GR.make_inputs(c)
    x, w, dy = inp["x"], inp["w"], inp["dy"]
    b = torch.linspace(-1, 1, N)
    assert GR.PATH_NAME[hip_lib.mmvae_linear_fwd_path(M, N, K, K, act, 0, 1, 1, 1)] == fwd
    assert GR.PATH_NAME[hip_lib.mmvae_linear_bwd_path(M, N, K, K, act, _DACT[act], 0, 1, 1, 1, 1, None, None)] == bwd
    xg, wg, bg = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = ops.linear(xg, wg, bg, act)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    d = [t.double() for t in (x, w, b, dy)]
    ref = GR.linear_fwd_reference(d[0], d[1], d[2], None, act)
    bounds = GR.linear_fwd_reference(d[0], d[1], d[2], None, act, _f=GR.gemm_bounds)
    aux = d[0] if _DACT[act] else None
    ref.update(GR.linear_bwd_reference(d[3], d[0], d[1], aux, x_act=act, ep=_DACT[act]))
    bounds.update(GR.linear_bwd_reference(d[3], d[0], d[1], aux, x_act=act, ep=_DACT[act], _f=GR.gemm_bounds))
    _check(f"linear-{M}x{N}x{K}-a{act}", {"y": y, "dx": xg.grad, "dw": wg.grad, "db": bg.grad}, ref, bounds)


@pytest.mark.parametrize("M,K,C,G,act,paths", [(17, 20, 3, 12, GR.ACT_SILU, ("R16_16_VS", "R16_16_VV", "R16_16_SS")),
                                               (300, 33, 2, 9, GR.ACT_RELU, ("R16_16_SS", "R16_16_SS", "RSPLIT_16"))])
def test_ops_linear_kn_autograd(hip_lib, M, K, C, G, act, paths):
    """ops.LinearKN (weight stored (K, N)): forward with A k-major and B n-major, data gradient with both k-major, weight
    gradient with A m-major through a caller-chosen split request and mmvae_gemm_splits"""
    from multimodal_vae_comparison_amd import ops
    N = C * G
    g = torch.Generator().manual_seed(M * 31 + K)
    x, w, dy = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) / K ** 0.5, torch.randn(M, N, generator=g)
    tiles = ((K + 31) // 32) * ((N + 31) // 32)
    want = max(1, min(64, 512 // max(tiles, 1), (M + 127) // 128))
    nz = ctypes.c_int(0)
    q = hip_lib.mmvae_gemm_path
    got_paths = (q(M, N, K, K, 1, N, 1, N, act, 0, 0, 0, 1, 0, 1, 1, None, None),
                 q(M, K, N, N, 1, 1, N, K, 0, 0, _DACT[act], 0, 1, 0, 1, 1, None, None),
                 q(K, N, M, 1, K, N, 1, N, act, 0, 0, 0, want, 0, 1, 1, ctypes.byref(nz), None))
    assert tuple(GR.PATH_NAME[p] for p in got_paths) == paths
    assert nz.value == hip_lib.mmvae_gemm_splits(K, N, M, want)
    xg, wg = (t.to(DEV).requires_grad_(True) for t in (x, w))
    y = ops.LinearKN.apply(xg, wg.view(K, C, 1, G), None, act, None, None)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    xd, wd, dyd = x.double(), w.double(), dy.double()
    aux = xd if _DACT[act] else None
    ref, bounds = {}, {}
    for f, out in ((GR.gemm_reference, ref), (GR.gemm_bounds, bounds)):
        out["y"] = f(xd, wd, a_act=act)["C"]
        out["dx"] = f(dyd, wd.t(), None, aux, ep=_DACT[act])["C"]
        out["dw"] = f(xd.t(), dyd, a_act=act)["C"]
    _check(f"linear_kn-{M}x{N}x{K}-a{act}", {"y": y, "dx": xg.grad, "dw": wg.grad.view(K, N)}, ref, bounds)
