"""GPU parity of the product-of-experts fusion (csrc/latent.hip: mmvae_poe_reparam_kl_fwd / _bwd / _bwd_acc, through
ops.poe_reparam_kl) against the float64 restatement of tests/poe_reference.py (pinned to torch on the CPU by tests/
test_poe_reference_host.py), PART BY PART: the joint mean, the joint variance, every KL row, every z_i, every expert's
dmu half and dlv (raw heads: du) half and dtheta are each held to their OWN float64 maximum -- max |dlv| is 60 to 1000
times max |dmu| (the -gk / lv term), so one bound on the packed gradient lets a mean gradient be 1 % off.  KL rows outside
the mask and gradient columns outside a column range must be exactly 0.

Both kernel families (poe_*_fast_kernel<E, NZ>: D <= 64, E <= 3, n_z <= 3; poe_fwd / poe_bwd_kernel: everything else) at
every bound of theirs, raw heads (softmax + 1e-6 in the kernel), the three with_prior modes, column ranges, more rows
than waves (B > 512: a wave's second and third row), absent upstream gradients, the prior gradient's three ways out (the
last-workgroup fold, accumulation into a preset tensor, the second launch), in-kernel noise in the generic kernels, and
the host entries' refusals.

Tolerances (poe_reference.TOL_*): joint and z 1e-5, KL rows 2e-5, gradients 5e-5 -- the numbers test_hip_ops always
used for this op.  The restatement itself evaluated in float32 on the CPU is within 5e-7 of float64 on every part
(test_reference_in_float32_is_within_5e_7_of_float64), which leaves 20 to 100 times that for the device's expf / logf
and the order of the sums.

Worst error of each part over this file on an MI355X (printed at the end of a run with -s), of its float64 maximum:
    joint 1.9e-7, z 2.0e-7, kl rows 2.2e-7, dmu 4.7e-7, dlv 4.1e-7, du 2.2e-7, dtheta 6.7e-7
-- float32 rounding, 20 to 100 times inside the bounds.  The one case that was outside: raw heads of ONE column (D = 1),
du = 6e-8 dlv where the function is constant in u and du is 0: the softmax backward's dot product takes s = lv - 1e-6,
which is rounded.  The kernels now write 0 for that width and keep their arithmetic at every other one bit for bit
(csrc/latent.hip)."""
import ctypes

import pytest
import torch

import poe_reference as R

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


def run_op(ops, c, inp, use_kl=True, use_z=None, gtheta=None, theta_grad=True, backward=True):
    """the op on the device for upstream gradients gkl (use_kl) and gz[i] (i in use_z; default: all)
    -> joint, kl, z, dheads, dtheta (None without theta_grad)"""
    use_z = range(c.n_z) if use_z is None else use_z
    heads = [h.to(DEV).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].to(DEV).requires_grad_(theta_grad and gtheta is None)
    joint, kl, z = ops.poe_reparam_kl(theta, heads, [e.to(DEV) for e in inp["eps"]], c.with_prior, c.kl_mask, gtheta,
                                      cols=c.cols, raw=c.raw)
    terms = [(kl * inp["gkl"].to(DEV)).sum()] if use_kl and c.kl_mask else []
    terms += [(z[i] * inp["gz"][i].to(DEV)).sum() for i in use_z]
    if not (backward and terms):
        return joint, kl, z, None, None
    torch.stack(terms).sum().backward()
    return joint, kl, z, [h.grad for h in heads], theta.grad


def whole_op(ops, c):
    inp, ref = reference(c)
    joint, kl, z, dheads, dtheta = run_op(ops, c, inp, theta_grad=not c.theta0)
    p = R.Parts(c.name, WORST)
    R.check_forward(p, c, joint, kl, z, ref)
    assert (dheads is None) == (ref["dheads"] is None)
    if dheads is not None:
        R.check_backward(p, c, dheads, dtheta, ref)
    p.done()


@pytest.mark.parametrize("c", R.FAST_CASES, ids=repr)
def test_fast_kernels_match_float64(ops, c):
    """poe_fwd_fast_kernel / poe_bwd_fast_kernel<E, NZ>: D at 1, inside, one below and at the 64 lanes; the corner
    instantiations; one row, fewer rows than a workgroup's waves, a wave's second row (513) and third (1100); every
    form of the KL mask; with and without the prior expert"""
    assert c.fast
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.GENERIC_CASES, ids=repr)
def test_generic_kernels_match_float64(ops, c):
    """poe_fwd_kernel / poe_bwd_kernel: every column slot (D up to 256), E > 3 and n_z > 3 at a small D, every bound at
    its limit at once, a wave's second and third row, the per-expert KL terms (gk[e]) under every form of the mask"""
    assert not c.fast
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.RAW_CASES, ids=repr)
def test_raw_heads_match_float64(ops, c):
    """raw=True, the form the PoE and MoPoE objectives call: softmax + 1e-6 and its backward du = s (dlv - sum s dlv)
    inside both kernel families; `spike`: one row of expert 0 whose softmax saturates (lv = 1e-6 in every other column)"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.PASS_THROUGH_CASES, ids=repr)
def test_pass_through_posterior_matches_float64(ops, c):
    """with_prior = 2 (MoE, DMVAE's shared and private parts, the unimodal VAE): z = mu + lv eps, KL of N(mu, lv);
    theta0: the zero row those callers pass for the N(0, 1) prior, without a gradient"""
    whole_op(ops, c)


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("c", R.COLUMN_CASES, ids=repr)
def test_column_ranges_match_float64(ops, monkeypatch, c, share):
    """cols = (col0, D) of a wider head (ld > D, col0 > 0), as the joint and as the pass-through posterior, with one
    gradient tensor per call and with the shared one (mmvae_poe_reparam_kl_bwd_acc): the columns outside are exactly 0"""
    monkeypatch.setattr(ops.GradReducer, "share_packed_grads", share)
    whole_op(ops, c)
    assert not ops.GradReducer.packed_grads


@pytest.mark.parametrize("c", R.FAMILY_CASES, ids=repr)
@pytest.mark.parametrize("use_kl,use_z", [(True, ()), (True, (1,)), (False, (0, 1, 2))],
                         ids=["kl-only", "kl-and-z1", "z-only"])
def test_absent_upstream_gradients(ops, c, use_kl, use_z):
    """every dz None, two of three dz None, dkl None: the backward's stand-ins are zeros, not stale memory"""
    inp, _ = reference(c)
    ref = R.run_reference(c, inp, use_kl=use_kl, use_z=use_z)
    _, _, _, dheads, dtheta = run_op(ops, c, inp, use_kl=use_kl, use_z=use_z)
    p = R.Parts(f"{c.name} [kl {use_kl}, z {list(use_z)}]", WORST)
    R.check_backward(p, c, dheads, dtheta, ref)
    p.done()


@pytest.mark.parametrize("c", R.THETA_CASES, ids=repr)
def test_prior_gradient_every_way_out(ops, monkeypatch, c):
    """dtheta of one-launch backward passes twice in a row (the elected workgroup left the ticket at zero), accumulated
    into a preset tensor of ones, and from the second launch (ticket == NULL -> poe_theta_kernel)"""
    inp, ref = reference(c)
    p = R.Parts(c.name, WORST)
    assert ops._poe_ticket(torch.device(DEV, torch.cuda.current_device())) is not None
    for rep in range(2):
        _, _, _, dheads, dtheta = run_op(ops, c, inp)
        R.check_backward(p, c, dheads, dtheta, ref, f"dtheta (one launch, pass {rep})")
    gtheta = torch.ones(1, c.D, device=DEV)
    _, _, _, dheads, none = run_op(ops, c, inp, gtheta=gtheta)
    assert none is None
    R.check_backward(p, c, dheads, gtheta - 1, ref, "dtheta (accumulated into ones)")
    with monkeypatch.context() as m:
        m.setattr(ops, "_poe_ticket", lambda dev: None)
        _, _, _, dheads, dtheta = run_op(ops, c, inp)
        R.check_backward(p, c, dheads, dtheta, ref, "dtheta (two launches)")
        gtheta = torch.ones(1, c.D, device=DEV)
        _, _, _, dheads, _ = run_op(ops, c, inp, gtheta=gtheta)
        R.check_backward(p, c, dheads, gtheta - 1, ref, "dtheta (two launches, accumulated into ones)")
    p.done()


@pytest.mark.parametrize("n_z,E,D,B", R.NOISE_CASES)
def test_generic_kernel_draws_its_own_noise(ops, n_z, E, D, B):
    """rng=state in poe_fwd_kernel (test_hip_ops.test_poe_draws_its_own_noise holds the fast kernels): bit-identical z,
    kl and gradients to drawing ops.randn((n_z, B, D), state) first, and the generator advances by exactly one draw"""
    c = R.Case("noise", E, n_z, D, B, 1, (1 << (E + 1)) - 1)
    assert not c.fast
    inp = R.make_inputs(c)
    res = []
    for fused in (False, True):
        state = torch.tensor([1234567, 5, 0], dtype=torch.int32, device=DEV)
        heads = [h.to(DEV).requires_grad_(True) for h in inp["heads"]]
        theta = inp["theta"].to(DEV).requires_grad_(True)
        if fused:
            _, kl, z = ops.poe_reparam_kl(theta, heads, n_z, 1, c.kl_mask, rng=state)
        else:
            eps = list(ops.randn((n_z, B, D), state).unbind(0))
            _, kl, z = ops.poe_reparam_kl(theta, heads, eps, 1, c.kl_mask)
        ((kl * inp["gkl"].to(DEV)).sum() + (torch.stack(z) * inp["gz"].to(DEV)).sum()).backward()
        assert state.tolist() == [1234567, 6, 0]
        res.append((kl, torch.stack(z), *[h.grad for h in heads], theta.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][1].detach().std()) > 0.1


# ---------------------------------------------------------------------------------------------
# refusals: return codes of the host entries; nothing is launched
# ---------------------------------------------------------------------------------------------
def _entries(hip_lib, H, E, with_prior, n_z, kl_mask, D, ld=None, raw=0, acc_packed=0, no_kl=False):
    """-> (forward's return code, backward's) for buffers that would hold the call, and whether anything was written"""
    B = 3
    ld = 2 * D if ld is None else ld
    n = max(E, n_z, 1)
    heads = torch.full((n, B, max(ld, 2 * D)), 0.25, device=DEV)
    rest = torch.full((4, n, B, D), 0.5, device=DEV)              # eps, z, dz and the forward's outputs
    dheads = torch.full_like(heads, 0.5)
    theta = torch.zeros(1, D, device=DEV)
    joint = torch.full((2, B, D), 0.5, device=DEV)
    kl = torch.full((E + 1, B), 0.5, device=DEV)
    dtheta = torch.full((1, D), 0.5, device=DEV)
    ws = torch.full((H.lib().mmvae_poe_ws_floats(B, D),), 0.5, device=DEV)
    fa, ba = H.PoeFwdArgs(), H.PoeBwdArgs()
    for e in range(min(n, H.MAX_EXPERTS)):
        fa.mu[e] = ba.mu[e] = heads[e].data_ptr()
        fa.lv[e] = ba.lv[e] = heads[e].data_ptr() + 4 * D
        fa.eps[e] = ba.eps[e] = rest[0, e].data_ptr()
        fa.z[e] = rest[1, e].data_ptr()
        ba.dz[e] = rest[2, e].data_ptr()
        ba.dmu[e] = dheads[e].data_ptr()
        ba.dlv[e] = dheads[e].data_ptr() + 4 * D
    rf = hip_lib.mmvae_poe_reparam_kl_fwd(ctypes.byref(fa), H.ptr(theta), H.ptr(joint), None if no_kl else H.ptr(kl), E,
                                          with_prior, n_z, kl_mask, B, D, ld, raw, None, H.stream())
    rb = hip_lib.mmvae_poe_reparam_kl_bwd_acc(ctypes.byref(ba), H.ptr(theta), H.ptr(kl), H.ptr(dtheta), H.ptr(ws), None, E,
                                              with_prior, n_z, kl_mask, B, D, ld, raw, 0, acc_packed, H.stream())
    torch.cuda.synchronize()
    written = any(bool((t != 0.5).any()) for t in (rest, dheads, joint, kl, dtheta, ws))
    return rf, rb, written


def test_refusals(hip_lib):
    from multimodal_vae_comparison_amd import hipops as H
    from multimodal_vae_comparison_amd import ops
    ARG, UNSUPPORTED = H.ERR_ARG, H.ERR_UNSUPPORTED
    # (what, expected forward code, expected backward code, arguments); None: that entry has no such check to make
    table = [("D = 257", UNSUPPORTED, UNSUPPORTED, dict(E=2, with_prior=1, n_z=1, kl_mask=0b111, D=257)),
             ("E = 9", UNSUPPORTED, UNSUPPORTED, dict(E=9, with_prior=1, n_z=1, kl_mask=0, D=8)),
             ("n_z = 9", UNSUPPORTED, UNSUPPORTED, dict(E=1, with_prior=1, n_z=9, kl_mask=0, D=8)),
             ("with_prior = 2 with E = 2", ARG, ARG, dict(E=2, with_prior=2, n_z=1, kl_mask=0, D=8)),
             ("kl_mask without kl", ARG, None, dict(E=2, with_prior=1, n_z=1, kl_mask=0b100, D=8, no_kl=True)),
             ("ld_in < D", ARG, ARG, dict(E=2, with_prior=1, n_z=1, kl_mask=0, D=8, ld=7)),
             ("acc_packed with raw heads", None, ARG, dict(E=2, with_prior=1, n_z=1, kl_mask=0, D=8, raw=1, acc_packed=1)),
             ("raw heads with with_prior = 2", ARG, ARG, dict(E=1, with_prior=2, n_z=1, kl_mask=0b10, D=8, raw=1)),
             ("raw heads with with_prior = 2 (generic)", ARG, ARG, dict(E=1, with_prior=2, n_z=1, kl_mask=0b10, D=70, raw=1))]
    bad = []
    for what, want_f, want_b, kw in table:
        rf, rb, written = _entries(hip_lib, H, **kw)
        if want_f is not None and rf != want_f:
            bad.append(f"{what}: forward returned {rf}, not {want_f}")
        if want_b is not None and rb != want_b:
            bad.append(f"{what}: backward returned {rb}, not {want_b}")
        if written and want_f is not None and want_b is not None:
            bad.append(f"{what}: something was launched")
    assert not bad, "; ".join(bad)
    # the same call with nothing wrong with it is accepted (the table above tests the refusals, not the harness)
    assert _entries(hip_lib, H, E=2, with_prior=1, n_z=1, kl_mask=0b111, D=8) == (0, 0, True)
    heads = [torch.randn(3, 16, device=DEV)]
    with pytest.raises(AssertionError, match="pass-through"):
        ops.poe_reparam_kl(torch.zeros(1, 8, device=DEV), heads, [torch.randn(3, 8, device=DEV)], 2, 0b10, raw=True)
