"""GPU parity of the mixture-of-experts prior (csrc/mixprior.hip: mmvae_mixprior_fwd / _bwd, through ops.mixprior_fusion)
against the float64 restatement of tests/mixprior_reference.py (pinned to torch.distributions on the CPU by tests/
test_mixprior_reference_host.py), PART BY PART: every expert's z, the kl_mix rows, the kl_std rows, every expert's dmu half
and dsigma (raw heads: du) half and dtheta are each held to their OWN float64 maximum, every kl_mix ENTRY to 2e-5 max(1,
|entry|) absolute and the responsibilities to 1e-5 absolute.

Every column slot (D = 1, 8, 63, 64, 65, 256), raw heads on and off, E = 1, 2, 3, 5, 8 (and E = 8 at D = 256), one row,
fewer rows than two workgroups, 37 rows, more rows than waves (1100 > 2 x 512), theta zero and random, a raw-head row whose
softmax saturates (scale 1e-6), scales of 1e-5, the far family (independent means: every responsibility saturated); what
is exact -- one expert, one column, no KL gradient --, one absent z gradient, accumulation into a preset prior gradient,
bit-reproducibility, the closed-form rows against ops.poe_reparam_kl, and the host entries' refusals.  The inputs overlap
(mixprior_reference asserts it): the kl_mix gradient is not the exact zero of saturated responsibilities.

Tolerances (poe_reference.TOL_*, the project's for this kind of op): z 1e-5, KL 2e-5, gradients 5e-5.  The restatement
itself evaluated in float32 on the CPU is within 4.9e-6 of float64 on every part (tests/test_mixprior_reference_host.py).

Worst error of each part over this file on an MI355X (printed at the end of a run with -s), of its float64 maximum:
    z 5.4e-8, kl_mix rows 1.4e-6, kl_std rows 1.8e-7, dmu 1.5e-6, dsigma 1.1e-6, du 5.8e-6, dtheta 5.6e-7
    every kl_mix entry over max(1, |entry|): 3.7e-6; resp, absolute: 1.3e-6
-- float32 rounding, 5 to 180 times inside the bounds."""
import ctypes
import math

import pytest
import torch

import mixprior_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}
_REF = {}


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    yield ops
    print("\nworst error of each part: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


def reference(c):
    """(inputs, float64 outputs and gradients with every upstream gradient present) of a case: computed once"""
    if c.name not in _REF:
        inp = R.make_inputs(c)
        _REF[c.name] = (inp, R.run_reference(c, inp))
    return _REF[c.name]


def run_op(ops, c, inp, use_kl=True, use_z=True, gtheta=None):
    """the op on the device for upstream gradients gkl (use_kl) and gz (use_z: True, False or the experts whose z has one)
    -> z, kl, resp, dheads, dtheta"""
    heads = [h.to(DEV).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].to(DEV).requires_grad_(gtheta is None)
    z, kl, resp = ops.mixprior_fusion(theta, heads, inp["eps"].to(DEV), gtheta, raw=c.raw)
    assert not resp.requires_grad and isinstance(z, tuple) and len(z) == c.E
    with_z = range(c.E) if use_z is True else (() if use_z is False else use_z)
    terms = [(z[e] * inp["gz"][e].to(DEV)).sum() for e in with_z]
    if use_kl:
        terms.append((kl * inp["gkl"].to(DEV)).sum())
    torch.stack(terms).sum().backward()
    return z, kl, resp, [h.grad for h in heads], theta.grad


def whole_op(ops, c):
    inp, ref = reference(c)
    z, kl, resp, dheads, dtheta = run_op(ops, c, inp)
    p = R.Parts(c.name, WORST)
    R.check_forward(p, c, z, kl, resp, ref)
    R.check_backward(p, c, dheads, dtheta, ref)
    p.done()
    return kl, resp


@pytest.mark.parametrize("c", R.WIDTH_CASES, ids=repr)
def test_every_width_matches_float64(ops, c):
    """D at 1, inside, one below, at and one above the 64 lanes and at the limit, raw heads on and off; D = 1 raw: du is
    exactly 0, D = 1: dtheta is exactly 0"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.EXPERT_CASES, ids=repr)
def test_every_expert_count_matches_float64(ops, c):
    """E = 1, 2, 3, 5, 8 at D = 8 and both limits at once (E = 8, D = 256); E = 1: kl_mix is exactly 0, resp exactly 1"""
    _, resp = whole_op(ops, c)
    if c.E == 1:
        assert bool((resp == 1).all())


@pytest.mark.parametrize("c", R.ROW_CASES, ids=repr)
def test_every_row_count_matches_float64(ops, c):
    """one row, fewer rows than two workgroups' waves, 37 rows, and 1100 rows on 512 waves: a wave's second and third row"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.SPIKE_CASES + R.THETA0_CASES + R.TINY_CASES, ids=repr)
def test_saturated_softmax_zero_theta_and_tiny_scales_match_float64(ops, c):
    """`spike`: one raw-head row of expert 0 whose softmax saturates (scale 1e-6 in every other column: u_mj reaches 1e6
    and its square 1e12 there); theta0: the prior N(0, 1) every model starts from; scales of 1e-5, where the absolute
    log-densities would lose the KL (test_mixprior_reference_host.test_plain_form_in_float32_does_not)"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.FAR_CASES, ids=repr)
def test_far_family_takes_the_saturated_path(ops, c):
    """independent means: every sample's own responsibility is 1, kl_mix is log E and only the closed-form rows and the
    samples carry a gradient"""
    kl, resp = whole_op(ops, c)
    own = torch.stack([resp[m, m] for m in range(c.E)])
    assert bool((own == 1).all()) and float((kl[:c.E] - math.log(c.E)).abs().max()) <= 1e-6


@pytest.mark.parametrize("c", R.FAMILY_CASES + [R.Case(2, 1, R.B0, raw=True)], ids=repr)
def test_without_kl_gradient_the_samples_are_the_whole_backward(ops, c):
    """no dkl: dmu_m IS gz_m and (heads that are not raw) dsigma_m IS gz_m * eps_m as one float32 product, bit for bit;
    dtheta is exactly 0; one column of raw heads: du is exactly 0"""
    inp, _ = reference(c)
    _, _, _, dheads, dtheta = run_op(ops, c, inp, use_kl=False)
    for e in range(c.E):
        gz = inp["gz"][e].to(DEV)
        dmu, dsg = R.split_packed(dheads[e], c.D)
        assert torch.equal(dmu, gz), e
        if not c.raw:
            assert torch.equal(dsg, gz * inp["eps"][e].to(DEV)), e      # (one float32 multiply, as the kernel forms it)
        elif c.D == 1:
            assert not bool(dsg.any()), e
    assert dtheta is not None and not bool(dtheta.any())


@pytest.mark.parametrize("c", R.FAMILY_CASES, ids=repr)
@pytest.mark.parametrize("use_kl,use_z", [(False, True), (True, False), (True, (0, 2)), (False, (1,))],
                         ids=["dkl-none", "dz-none", "dz1-none", "only-dz1"])
def test_absent_upstream_gradients(ops, c, use_kl, use_z):
    """dkl None, every dz None, ONE expert's dz None, only one present: an absent gradient counts as zeros, not as stale
    memory"""
    inp, _ = reference(c)
    ref = R.run_reference(c, inp, use_kl=use_kl, use_z=use_z)
    _, _, _, dheads, dtheta = run_op(ops, c, inp, use_kl=use_kl, use_z=use_z)
    p = R.Parts(f"{c.name} [kl {use_kl}, z {use_z}]", WORST)
    if use_kl:
        R.check_backward(p, c, dheads, dtheta, ref)
    else:
        R.check_backward(p, c, dheads, None, ref)
        p.exact_zero("dtheta (no KL gradient: the prior is not reached)", dtheta)
    p.done()
    if not use_kl:      # an expert without a z gradient gets exactly nothing
        for e in set(range(c.E)) - set(range(c.E) if use_z is True else use_z):
            assert not bool(dheads[e].any()), e


@pytest.mark.parametrize("c", R.THETA_CASES, ids=repr)
def test_prior_gradient_accumulates_and_the_op_is_bit_reproducible(ops, c):
    """two runs in a row give identical bits (every sum in one fixed order: no atomics, no election); gtheta preset to
    ones: the fold ADDS to the ones"""
    inp, ref = reference(c)
    p = R.Parts(c.name, WORST)
    runs = [run_op(ops, c, inp) for _ in range(2)]
    for a, b in zip(list(runs[0][0]) + list(runs[0][1:3]) + runs[0][3] + [runs[0][4]],
                    list(runs[1][0]) + list(runs[1][1:3]) + runs[1][3] + [runs[1][4]]):
        assert torch.equal(a, b)
    R.check_backward(p, c, runs[0][3], runs[0][4], ref)
    gtheta = torch.ones(1, c.D, device=DEV)
    _, _, _, dheads, none = run_op(ops, c, inp, gtheta=gtheta)
    assert none is None
    R.check_backward(p, c, dheads, gtheta - 1, ref, "dtheta (accumulated into ones)")
    assert float((gtheta - 1 - runs[0][4]).abs().max()) <= 2e-7 * float(1 + runs[0][4].abs().max())
    p.done()


@pytest.mark.parametrize("c", R.FAMILY_CASES + [R.Case(2, 256, 7)], ids=repr)
def test_closed_form_rows_are_the_mixture_of_experts_own(ops, c):
    """kl_std row m against the row ops.poe_reparam_kl gives MOE.objective for the same head (one expert, no product,
    kl_mask 0b10), and z_m against its sample: within TOL_KL / TOL_Z of each other"""
    inp, _ = reference(c)
    theta = inp["theta"].to(DEV)
    heads = [h.to(DEV) for h in inp["heads"]]
    with torch.no_grad():
        z, kl, _ = ops.mixprior_fusion(theta, heads, inp["eps"].to(DEV), raw=c.raw)
        for m in range(c.E):
            head = heads[m]
            if c.raw:
                head = torch.cat([head[:, :c.D], torch.softmax(head[:, c.D:], -1) + 1e-6], -1)
            _, kl_moe, z_moe = ops.poe_reparam_kl(theta, [head], [inp["eps"][m].to(DEV)], 2, 0b10)
            assert R.rel_err(kl[c.E + m], kl_moe[1]) <= R.TOL_KL, m
            assert R.rel_err(z[m], z_moe[0]) <= R.TOL_Z, m


# ---------------------------------------------------------------------------------------------
# refusals: return codes of the host entries; nothing is launched
# ---------------------------------------------------------------------------------------------
def _entries(hip_lib, H, E, D, ld=None, null=None):
    """-> (forward's return code, backward's, whether anything was written) for buffers that would hold the call; null:
    the name of one pointer handed over as NULL"""
    B = 3
    ld = 2 * D if ld is None else ld
    n = max(min(E, H.MAX_EXPERTS), 1)
    heads = torch.full((n, B, max(ld, 2 * D)), 0.25, device=DEV)
    dheads = torch.full_like(heads, 0.5)
    rest = torch.full((3, n, B, D), 0.5, device=DEV)              # eps, z, dz
    theta = torch.zeros(1, D, device=DEV)
    kl = torch.full((2 * E, B), 0.5, device=DEV)
    resp = torch.full((max(E, 1), max(E, 1), B), 0.5, device=DEV)
    dtheta = torch.full((1, D), 0.5, device=DEV)
    ws = torch.full((4 * D,), 0.5, device=DEV)
    fa, ba = H.PoeFwdArgs(), H.PoeBwdArgs()
    for e in range(n):
        fa.mu[e] = ba.mu[e] = heads[e].data_ptr()
        fa.lv[e] = ba.lv[e] = heads[e].data_ptr() + 4 * D
        fa.eps[e] = ba.eps[e] = rest[0, e].data_ptr()
        fa.z[e] = rest[1, e].data_ptr()
        ba.dz[e] = rest[2, e].data_ptr()
        ba.dmu[e] = dheads[e].data_ptr()
        ba.dlv[e] = dheads[e].data_ptr() + 4 * D
    ptrs = {"theta": H.ptr(theta), "kl": H.ptr(kl), "resp": H.ptr(resp), "ws": H.ptr(ws), "args": True}
    if null in ptrs:
        ptrs[null] = None
    elif null is not None:      # a table entry of expert 1
        for table in (fa, ba):
            if hasattr(table, null):
                getattr(table, null)[1] = None
    rf = hip_lib.mmvae_mixprior_fwd(ctypes.byref(fa) if ptrs["args"] else None, ptrs["theta"], ptrs["kl"], ptrs["resp"], E, B,
                                    D, ld, 0, H.stream())
    rb = hip_lib.mmvae_mixprior_bwd(ctypes.byref(ba) if ptrs["args"] else None, ptrs["theta"], ptrs["resp"], H.ptr(kl),
                                    H.ptr(dtheta), ptrs["ws"], E, B, D, ld, 0, 0, H.stream())
    torch.cuda.synchronize()
    written = any(bool((t != 0.5).any()) for t in (rest, dheads, kl, resp, dtheta, ws))
    return rf, rb, written


def test_refusals(hip_lib, ops):
    from multimodal_vae_comparison_amd import hipops as H
    assert _entries(hip_lib, H, E=2, D=257) == (H.ERR_UNSUPPORTED, H.ERR_UNSUPPORTED, False)
    assert _entries(hip_lib, H, E=9, D=8) == (H.ERR_UNSUPPORTED, H.ERR_UNSUPPORTED, False)
    assert _entries(hip_lib, H, E=2, D=8, ld=7) == (H.ERR_ARG, H.ERR_ARG, False)
    assert _entries(hip_lib, H, E=0, D=8) == (H.ERR_ARG, H.ERR_ARG, False)
    # NULL pointers: the argument table, theta, resp and an expert's table entries refuse both ways
    for null in ("args", "theta", "resp", "mu", "lv", "eps"):
        assert _entries(hip_lib, H, E=2, D=8, null=null) == (H.ERR_ARG, H.ERR_ARG, False), null
    # ... those only one direction has refuse that one (the other runs and writes)
    assert _entries(hip_lib, H, E=2, D=8, null="kl")[0] == H.ERR_ARG and _entries(hip_lib, H, E=2, D=8, null="z")[0] == H.ERR_ARG
    for null in ("ws", "dmu", "dlv"):
        assert _entries(hip_lib, H, E=2, D=8, null=null)[:2] == (0, H.ERR_ARG), null
    # an expert's dz may be NULL: an absent gradient
    assert _entries(hip_lib, H, E=2, D=8, null="dz") == (0, 0, True)
    # the same call with nothing wrong with it is accepted, at both limits too
    assert _entries(hip_lib, H, E=2, D=8) == (0, 0, True)
    assert _entries(hip_lib, H, E=8, D=256) == (0, 0, True)
    # ... and the wrapper turns a refusal into an error
    for E, D in ((9, 8), (2, 257)):
        heads = [torch.randn(3, 2 * D, device=DEV) for _ in range(E)]
        with pytest.raises(RuntimeError, match="mmvae_mixprior_fwd failed: unsupported shape"):
            ops.mixprior_fusion(torch.zeros(1, D, device=DEV), heads, torch.randn(E, 3, D, device=DEV))
