"""GPU parity of the total-correlation fusion (csrc/tcfusion.hip: mmvae_tc_fusion_fwd / _bwd, through ops.tc_fusion)
against the float64 restatement of tests/tc_reference.py (pinned to torch.distributions on the CPU by tests/
test_tc_reference_host.py), PART BY PART: the joint mean, the joint variance, z, every KL row, every expert's dmu half and
dlv (raw heads: du) half and dtheta are each held to their OWN float64 maximum.

Every column slot (D = 1, 8, 63, 64, 65, 256), raw heads on and off, E = 1, 2, 3, 5, 8 (and E = 8 at D = 256), one row,
fewer rows than two workgroups, more rows than waves (1100 > 2 x 512: a wave's second and third row), a raw-head row
whose softmax saturates, theta zero and random, absent upstream gradients, accumulation into a preset prior gradient,
bit-reproducibility of the backward pass, and the host entries' refusals.

Tolerances (poe_reference.TOL_*, the project's for this kind of op): joint and z 1e-5, KL rows 2e-5, gradients 5e-5.  The
restatement itself evaluated in float32 on the CPU is within 1.7e-6 of float64 on every part
(test_reference_in_float32_is_within_2e_6_of_float64).  One expert (E = 1): the joint IS the expert, its KL row is
analytically 0 and is held to 2e-5 of the prior row's maximum, the gradient that flows through that row alone to 5e-5 of
the gradient through the prior row alone.

Worst error of each part over this file on an MI355X (printed at the end of a run with -s), of its float64 maximum:
    joint 2.0e-7, z 1.8e-7, kl rows 2.6e-7, dmu 5.0e-7, dlv 3.3e-7, du 5.3e-7, dtheta 4.8e-7
    one expert: kl[0] 1.4e-8 of the prior row's maximum; the gradient through kl[0] alone, of the gradient through the prior
    row: dmu 1.0e-15, dlv 2.4e-8, du 6.6e-8
-- float32 rounding, 20 to 100 times inside the bounds."""
import ctypes

import pytest
import torch

import tc_reference as R

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


def run_op(ops, c, inp, use_kl=True, use_z=True, rows=None, gtheta=None):
    """the op on the device for upstream gradients gkl (use_kl; rows: only these KL rows, through a mask of zeros) and gz
    (use_z) -> joint, kl, z, dheads, dtheta"""
    heads = [h.to(DEV).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].to(DEV).requires_grad_(gtheta is None)
    joint, kl, z = ops.tc_fusion(theta, heads, inp["eps"].to(DEV), gtheta, raw=c.raw)
    assert not joint.requires_grad
    terms = []
    if use_kl:
        gkl = inp["gkl"].clone()
        if rows is not None:
            keep = torch.zeros(c.E + 1, 1)
            keep[list(rows)] = 1
            gkl = gkl * keep
        terms.append((kl * gkl.to(DEV)).sum())
    if use_z:
        terms.append((z * inp["gz"].to(DEV)).sum())
    torch.stack(terms).sum().backward()
    return joint, kl, z, [h.grad for h in heads], theta.grad


def whole_op(ops, c):
    inp, ref = reference(c)
    joint, kl, z, dheads, dtheta = run_op(ops, c, inp)
    p = R.Parts(c.name, WORST)
    R.check_forward(p, c, joint, kl, z, ref)
    R.check_backward(p, c, dheads, dtheta, ref)
    p.done()


@pytest.mark.parametrize("c", R.WIDTH_CASES, ids=repr)
def test_every_width_matches_float64(ops, c):
    """D at 1, inside, one below, at and one above the 64 lanes and at the limit, raw heads on and off; D = 1 raw: du is
    exactly 0, D = 1: dtheta is exactly 0"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.EXPERT_CASES, ids=repr)
def test_every_expert_count_matches_float64(ops, c):
    """E = 1, 2, 3, 5, 8 at D = 8 and both limits at once (E = 8, D = 256)"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.ROW_CASES, ids=repr)
def test_every_row_count_matches_float64(ops, c):
    """one row, fewer rows than two workgroups' waves, and 1100 rows on 512 waves: a wave's second and third row"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.SPIKE_CASES + R.THETA0_CASES, ids=repr)
def test_saturated_softmax_and_zero_theta_match_float64(ops, c):
    """`spike`: one raw-head row of expert 0 whose softmax saturates (lv = 1e-6 in every other column); theta0: the prior
    N(0, 1) every model starts from"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.SINGLE_CASES, ids=repr)
def test_one_expert_row_and_its_gradient_are_zero(ops, c):
    """E = 1: the joint is the expert, kl[0] = 0 analytically (held to 2e-5 of the prior row's maximum by whole_op) and the
    gradient through kl[0] alone is 0: each part is held to 5e-5 of the same part of the gradient through the prior row"""
    whole_op(ops, c)
    inp, _ = reference(c)
    through_prior = R.run_reference(c, inp, use_z=False, rows=(1,))
    _, _, _, dheads, dtheta = run_op(ops, c, inp, use_z=False, rows=(0,))
    p = R.Parts(c.name + " [gradient through kl[0] alone]", WORST)
    for half, got, scale in zip(("dmu", "du" if c.raw else "dlv"), R.split_packed(dheads[0], c.D),
                                R.split_packed(through_prior["dheads"][0], c.D)):
        R.check_scaled(p, f"{half}[0]", got, torch.zeros_like(got), scale, R.TOL_GRAD, f"{half} (one expert)")
    p.exact_zero("dtheta (no gradient on the prior row)", dtheta)
    p.done()


@pytest.mark.parametrize("c", R.FAMILY_CASES, ids=repr)
@pytest.mark.parametrize("use_kl,use_z", [(False, True), (True, False), (True, True)], ids=["dkl-none", "dz-none", "both"])
def test_absent_upstream_gradients(ops, c, use_kl, use_z):
    """dkl None, dz None, both present: an absent gradient counts as zeros, not as stale memory"""
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


@pytest.mark.parametrize("c", R.THETA_CASES, ids=repr)
def test_prior_gradient_accumulates_and_the_backward_is_bit_reproducible(ops, c):
    """two backward passes in a row give identical bits (every sum in one fixed order: no atomics, no election); gtheta
    preset to ones: the fold ADDS to the ones"""
    inp, ref = reference(c)
    p = R.Parts(c.name, WORST)
    runs = [run_op(ops, c, inp) for _ in range(2)]
    for a, b in zip(runs[0][3] + [runs[0][4], runs[0][1], runs[0][2]], runs[1][3] + [runs[1][4], runs[1][1], runs[1][2]]):
        assert torch.equal(a, b)
    R.check_backward(p, c, runs[0][3], runs[0][4], ref)
    gtheta = torch.ones(1, c.D, device=DEV)
    _, _, _, dheads, none = run_op(ops, c, inp, gtheta=gtheta)
    assert none is None
    R.check_backward(p, c, dheads, gtheta - 1, ref, "dtheta (accumulated into ones)")
    assert float((gtheta - 1 - runs[0][4]).abs().max()) <= 2e-7 * float(1 + runs[0][4].abs().max())
    p.done()


# ---------------------------------------------------------------------------------------------
# refusals: return codes of the host entries; nothing is launched
# ---------------------------------------------------------------------------------------------
def _entries(hip_lib, H, E, D, ld=None):
    """-> (forward's return code, backward's, whether anything was written) for buffers that would hold the call"""
    B = 3
    ld = 2 * D if ld is None else ld
    n = max(E, 1)
    heads = torch.full((n, B, max(ld, 2 * D)), 0.25, device=DEV)
    dheads = torch.full_like(heads, 0.5)
    rest = torch.full((3, B, D), 0.5, device=DEV)              # eps, z, dz
    theta = torch.zeros(1, D, device=DEV)
    joint = torch.full((2, B, D), 0.5, device=DEV)
    kl = torch.full((E + 1, B), 0.5, device=DEV)
    dtheta = torch.full((1, D), 0.5, device=DEV)
    ws = torch.full((4 * D,), 0.5, device=DEV)
    fa, ba = H.TcFwdArgs(), H.TcBwdArgs()
    for e in range(min(n, H.MAX_EXPERTS)):
        fa.mu[e] = ba.mu[e] = heads[e].data_ptr()
        fa.lv[e] = ba.lv[e] = heads[e].data_ptr() + 4 * D
        ba.dmu[e] = dheads[e].data_ptr()
        ba.dlv[e] = dheads[e].data_ptr() + 4 * D
    rf = hip_lib.mmvae_tc_fusion_fwd(ctypes.byref(fa), H.ptr(theta), H.ptr(rest[0]), H.ptr(joint), H.ptr(kl), H.ptr(rest[1]),
                                     E, B, D, ld, 0, H.stream())
    rb = hip_lib.mmvae_tc_fusion_bwd(ctypes.byref(ba), H.ptr(theta), H.ptr(rest[0]), H.ptr(rest[2]), H.ptr(kl),
                                     H.ptr(dtheta), H.ptr(ws), E, B, D, ld, 0, 0, H.stream())
    torch.cuda.synchronize()
    written = any(bool((t != 0.5).any()) for t in (rest, dheads, joint, kl, dtheta, ws))
    return rf, rb, written


def test_refusals(hip_lib, ops):
    from multimodal_vae_comparison_amd import hipops as H
    assert _entries(hip_lib, H, E=2, D=257) == (H.ERR_UNSUPPORTED, H.ERR_UNSUPPORTED, False)
    assert _entries(hip_lib, H, E=9, D=8) == (H.ERR_UNSUPPORTED, H.ERR_UNSUPPORTED, False)
    assert _entries(hip_lib, H, E=2, D=8, ld=7) == (H.ERR_ARG, H.ERR_ARG, False)
    assert _entries(hip_lib, H, E=0, D=8) == (H.ERR_ARG, H.ERR_ARG, False)
    # the same call with nothing wrong with it is accepted, at both limits too
    assert _entries(hip_lib, H, E=2, D=8) == (0, 0, True)
    assert _entries(hip_lib, H, E=8, D=256) == (0, 0, True)
    # ... and the wrapper turns a refusal into an error
    for E, D in ((9, 8), (2, 257)):
        heads = [torch.randn(3, 2 * D, device=DEV) for _ in range(E)]
        with pytest.raises(RuntimeError, match="mmvae_tc_fusion_fwd failed: unsupported shape"):
            ops.tc_fusion(torch.zeros(1, D, device=DEV), heads, torch.randn(3, D, device=DEV))
