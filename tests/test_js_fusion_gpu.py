"""GPU parity of the Jensen-Shannon fusion (csrc/jsfusion.hip: mmvae_js_fusion_fwd / _bwd, through ops.js_fusion) against
the float64 restatement of tests/js_reference.py (pinned to torch.distributions on the CPU by tests/
test_js_reference_host.py), PART BY PART: the dynamic prior's mean and scale, z, every KL row, every expert's dmu half and
dsigma (raw heads: du) half and dtheta are each held to their OWN float64 maximum, and at D >= 8 every KL ENTRY to its own
float64 value.

Every column slot (D = 1, 8, 63, 64, 65, 256), raw heads on and off, E = 1, 2, 3, 5, 8 (and E = 8 at D = 256), one row,
fewer rows than two workgroups, more rows than waves (1100 > 2 x 512), a raw-head row whose softmax saturates (scale 1e-6, P
at 1e12), theta zero and random; uniform weights, the prior at 0.5, unequal expert weights; rows in balanced chunks, all
on one expert, shuffled; what the selection does to the gradient bit for bit; an index no expert has; absent upstream
gradients, accumulation into a preset prior gradient, bit-reproducibility, and the host entries' refusals.

Tolerances (poe_reference.TOL_*, the project's for this kind of op): prior and z 1e-5, KL rows and entries 2e-5, gradients
5e-5.  The restatement itself evaluated in float32 on the CPU is within 2.4e-6 of float64 on every part (tests/
test_js_reference_host.py).

Worst error of each part over this file on an MI355X (printed at the end of a run with -s), of its float64 maximum:
    prior 2.4e-7, z 7.7e-8, kl rows 9.0e-7, dmu 7.5e-7, dsigma 5.3e-7, du 9.5e-7, dtheta 6.8e-7
    every KL entry on its own float64 value (D >= 8; the smallest entry over the file is 0.68): 1.0e-6
-- float32 rounding, 20 to 100 times inside the bounds."""
import ctypes

import pytest
import torch

import js_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}
_REF = {}


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    yield ops
    print("\nworst error of each part: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


def reference(c, weights="uniform", sel="chunks"):
    """(inputs, float64 outputs and gradients with every upstream gradient present) of a case: computed once"""
    key = (c.name, weights, sel)
    if key not in _REF:
        inp = R.make_inputs(c, weights, sel)
        _REF[key] = (inp, R.run_reference(c, inp))
    return _REF[key]


def run_op(ops, c, inp, use_kl=True, use_z=True, gtheta=None, sel_on_device=False):
    """the op on the device for upstream gradients gkl (use_kl) and gz (use_z) -> prior, kl, z, dheads, dtheta"""
    heads = [h.to(DEV).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].to(DEV).requires_grad_(gtheta is None)
    sel = inp["sel"].to(DEV) if sel_on_device else inp["sel"]
    prior, kl, z = ops.js_fusion(theta, heads, inp["eps"].to(DEV), sel, inp["weights"], gtheta, raw=c.raw)
    assert not prior.requires_grad
    terms = []
    if use_kl:
        terms.append((kl * inp["gkl"].to(DEV)).sum())
    if use_z:
        terms.append((z * inp["gz"].to(DEV)).sum())
    torch.stack(terms).sum().backward()
    return prior, kl, z, [h.grad for h in heads], theta.grad


def whole_op(ops, c, weights="uniform", sel="chunks"):
    inp, ref = reference(c, weights, sel)
    prior, kl, z, dheads, dtheta = run_op(ops, c, inp)
    p = R.Parts(f"{c.name} [{weights}, {sel}]", WORST)
    R.check_forward(p, c, prior, kl, z, ref)
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
    """`spike`: one raw-head row of expert 0 whose softmax saturates (scale 1e-6 in every other column: that expert's T is
    1e12 there and the dynamic prior's mean sits on its mean to rounding -- every KL entry of that row is still held to its
    own float64 value); theta0: the prior N(0, 1) every model starts from"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.FAMILY_CASES + R.SPIKE_CASES[:1], ids=repr)
@pytest.mark.parametrize("sel", R.SELECTIONS)
@pytest.mark.parametrize("weights", R.WEIGHTS)
def test_every_weighting_and_selection_matches_float64(ops, c, weights, sel):
    """uniform weights, the prior at 0.5, unequal expert weights x rows in balanced chunks, every row on the last expert, a
    shuffled assignment"""
    whole_op(ops, c, weights, sel)


@pytest.mark.parametrize("c", [R.Case(3, 32, R.B0), R.Case(3, 70, R.B0, raw=True)], ids=repr)
@pytest.mark.parametrize("sel", R.SELECTIONS)
def test_without_kl_gradient_the_selection_is_the_whole_backward(ops, c, sel):
    """no dkl: an unselected expert's gradient rows are exactly 0, a selected row's dmu IS gz and (heads that are not raw)
    its dsigma IS gz * eps as one float32 product, bit for bit; dtheta is exactly 0"""
    inp, _ = reference(c, "unequal", sel)
    _, _, _, dheads, dtheta = run_op(ops, c, inp, use_kl=False)
    gz = inp["gz"].to(DEV)
    gze = gz * inp["eps"].to(DEV)      # (one float32 multiply, as the kernel forms it)
    s = inp["sel"].to(DEV)
    for e in range(c.E):
        mine = (s == e).unsqueeze(1)
        dmu, dsg = R.split_packed(dheads[e], c.D)
        assert torch.equal(dmu, torch.where(mine, gz, torch.zeros_like(gz))), e
        if c.raw:      # (through the softmax the selected rows' du is no plain product; the others stay exactly 0)
            assert not bool(dsg[~mine.expand_as(dsg)].any()), e
        else:
            assert torch.equal(dsg, torch.where(mine, gze, torch.zeros_like(gze))), e
    assert dtheta is not None and not bool(dtheta.any())


@pytest.mark.parametrize("c", R.FAMILY_CASES, ids=repr)
def test_an_index_no_expert_has_selects_nothing(ops, c):
    """a device `sel` is taken as is: rows whose value lies outside [0, E) get a zero z row and send no z-gradient anywhere,
    while their KL rows (and every other row) still match"""
    inp, _ = reference(c)
    inp = dict(inp, sel=inp["sel"].clone())
    odd = [1, 6, 20, 36]
    inp["sel"][odd] = torch.tensor([c.E, -1, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    ref = R.run_reference(c, inp)
    prior, kl, z, dheads, dtheta = run_op(ops, c, inp, sel_on_device=True)
    assert not bool(z[odd].any()) and bool(z.any(1).sum() == c.B - len(odd))
    p = R.Parts(c.name + " [sel out of range on four rows]", WORST)
    R.check_forward(p, c, prior, kl, z, ref)
    R.check_backward(p, c, dheads, dtheta, ref)
    p.done()
    _, _, _, only_z, _ = run_op(ops, c, inp, use_kl=False, sel_on_device=True)
    for g in only_z:
        assert not bool(g[odd].any())
    # ... and the wrapper refuses the same values when they come from the host
    with pytest.raises(ValueError, match="sel"):
        run_op(ops, c, inp)


@pytest.mark.parametrize("c", R.FAMILY_CASES, ids=repr)
@pytest.mark.parametrize("use_kl,use_z", [(False, True), (True, False), (True, True)], ids=["dkl-none", "dz-none", "both"])
def test_absent_upstream_gradients(ops, c, use_kl, use_z):
    """dkl None, dz None, both present: an absent gradient counts as zeros, not as stale memory"""
    inp, _ = reference(c, "half", "shuffled")
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
    for a, b in zip(runs[0][3] + [runs[0][4], runs[0][0], runs[0][1], runs[0][2]],
                    runs[1][3] + [runs[1][4], runs[1][0], runs[1][1], runs[1][2]]):
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
def _entries(hip_lib, H, E, D, ld=None, weights=None):
    """-> (forward's return code, backward's, whether anything was written) for buffers that would hold the call"""
    B = 3
    ld = 2 * D if ld is None else ld
    n = max(E, 1)
    heads = torch.full((n, B, max(ld, 2 * D)), 0.25, device=DEV)
    dheads = torch.full_like(heads, 0.5)
    rest = torch.full((3, B, D), 0.5, device=DEV)              # eps, z, dz
    theta = torch.zeros(1, D, device=DEV)
    sel = torch.zeros(B, dtype=torch.int32, device=DEV)
    prior = torch.full((2, B, D), 0.5, device=DEV)
    kl = torch.full((E + 1, B), 0.5, device=DEV)
    dtheta = torch.full((1, D), 0.5, device=DEV)
    ws = torch.full((4 * D,), 0.5, device=DEV)
    weights = [1.0 / (E + 1)] * (E + 1) if weights is None else weights
    w = (ctypes.c_float * len(weights))(*weights)
    fa, ba = H.TcFwdArgs(), H.TcBwdArgs()
    for e in range(min(n, H.MAX_EXPERTS)):
        fa.mu[e] = ba.mu[e] = heads[e].data_ptr()
        fa.lv[e] = ba.lv[e] = heads[e].data_ptr() + 4 * D
        ba.dmu[e] = dheads[e].data_ptr()
        ba.dlv[e] = dheads[e].data_ptr() + 4 * D
    rf = hip_lib.mmvae_js_fusion_fwd(ctypes.byref(fa), w, H.ptr(theta), H.ptr(rest[0]), H.ptr(sel), H.ptr(prior), H.ptr(kl),
                                     H.ptr(rest[1]), E, B, D, ld, 0, H.stream())
    rb = hip_lib.mmvae_js_fusion_bwd(ctypes.byref(ba), w, H.ptr(theta), H.ptr(rest[0]), H.ptr(sel), H.ptr(rest[2]),
                                     H.ptr(kl), H.ptr(dtheta), H.ptr(ws), E, B, D, ld, 0, 0, H.stream())
    torch.cuda.synchronize()
    written = any(bool((t != 0.5).any()) for t in (rest, dheads, prior, kl, dtheta, ws))
    return rf, rb, written


def test_refusals(hip_lib, ops):
    from multimodal_vae_comparison_amd import hipops as H
    assert _entries(hip_lib, H, E=2, D=257) == (H.ERR_UNSUPPORTED, H.ERR_UNSUPPORTED, False)
    assert _entries(hip_lib, H, E=9, D=8) == (H.ERR_UNSUPPORTED, H.ERR_UNSUPPORTED, False)
    assert _entries(hip_lib, H, E=2, D=8, ld=7) == (H.ERR_ARG, H.ERR_ARG, False)
    assert _entries(hip_lib, H, E=0, D=8) == (H.ERR_ARG, H.ERR_ARG, False)
    # the weights: every one finite and >= 0, their sum > 0
    for bad in ([0.5, -0.1, 0.6], [0.5, float("nan"), 0.5], [0.5, float("inf"), 0.5], [0.0, 0.0, 0.0]):
        assert _entries(hip_lib, H, E=2, D=8, weights=bad) == (H.ERR_ARG, H.ERR_ARG, False), bad
    # the same call with nothing wrong with it is accepted, at both limits and with a weight of 0 too
    assert _entries(hip_lib, H, E=2, D=8) == (0, 0, True)
    assert _entries(hip_lib, H, E=2, D=8, weights=[0.5, 0.0, 0.5]) == (0, 0, True)
    assert _entries(hip_lib, H, E=8, D=256) == (0, 0, True)
    # ... and the wrapper turns a refusal into an error
    for E, D in ((9, 8), (2, 257)):
        heads = [torch.randn(3, 2 * D, device=DEV) for _ in range(E)]
        with pytest.raises(RuntimeError, match="mmvae_js_fusion_fwd failed: unsupported shape"):
            ops.js_fusion(torch.zeros(1, D, device=DEV), heads, torch.randn(3, D, device=DEV), [0] * 3, [1.0] * (E + 1))
    heads = [torch.randn(3, 16, device=DEV) for _ in range(2)]
    with pytest.raises(RuntimeError, match="mmvae_js_fusion_fwd failed: invalid argument"):
        ops.js_fusion(torch.zeros(1, 8, device=DEV), heads, torch.randn(3, 8, device=DEV), [0, 1, 1], [0.5, -0.1, 0.6])
