"""GPU parity of MMVAE+'s latent op (csrc/mmplus.hip: mmvae_mmplus_fwd / _bwd, through ops.mmplus_fusion) against the
float64 restatement of tests/mmplus_reference.py (pinned to torch.distributions on the CPU by tests/
test_mmplus_reference_host.py), PART BY PART: every decoder's input batch z[n], the kl_mix, kl_u and kl_w row blocks, every
head's dmu half and dsigma (raw heads: du) half over all W = D + P columns and dtheta are each held to their OWN float64
maximum, every kl_mix ENTRY to 2e-5 max(1, |entry|) absolute and the responsibilities to 1e-5 absolute.

(D, P) at (1, 1), (8, 4), (60, 10), (63, 1), (64, 64), (65, 8), (192, 64) -- one column each, the private block ending at,
starting at and straddling a 64-lane slot, D + P at the limit --, raw heads on and off, E = 1, 2, 3, 5, 8 (and E = 8 at
(192, 64)), one row, fewer rows than two workgroups, 37 rows, more rows than waves (1100 > 2 x 512), theta zero and random, a
raw-head row whose softmax saturates in a shared and in a private column, scales of 1e-5, the far family (independent means:
every responsibility saturated); what is exact -- one expert, one shared column, no KL gradient --, absent z gradients,
accumulation into a preset prior gradient, bit-reproducibility, the shared rows against ops.mixprior_fusion and the private
rows against ops.poe_reparam_kl, and the host entries' refusals.

Tolerances (poe_reference.TOL_*, mixprior_reference.TOL_RESP: the project's for this kind of op): z 1e-5, KL 2e-5, gradients
5e-5, resp 1e-5 absolute.

Worst error of each part over this file on an MI355X (printed at the end of a run with -s), of its float64 maximum:
    z 5.8e-8, kl_mix rows 2.6e-6, kl_u rows 1.9e-7, kl_w rows 1.8e-7, dmu 1.1e-6, dsigma 9.1e-7, du 1.3e-6, dtheta 5.3e-7
    every kl_mix entry over max(1, |entry|): 5.1e-6; resp, absolute: 1.2e-6
-- float32 rounding, 4 to 170 times inside the bounds."""
import ctypes
import math

import pytest
import torch

import mmplus_reference as R

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
    """the op on the device for upstream gradients gkl (use_kl) and gz (use_z: True, False or the decoders whose z has one)
    -> z, kl, resp, dheads, dtheta"""
    heads = [h.to(DEV).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].to(DEV).requires_grad_(gtheta is None)
    z, kl, resp = ops.mmplus_fusion(theta, heads, inp["eps_u"].to(DEV), inp["eps_w"].to(DEV), inp["eps_a"].to(DEV), c.D,
                                    c.aux, gtheta, raw=c.raw)
    assert not resp.requires_grad and isinstance(z, tuple) and len(z) == c.E
    with_z = range(c.E) if use_z is True else (() if use_z is False else use_z)
    terms = [(z[n] * inp["gz"][n].to(DEV)).sum() for n in with_z]
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
    return z, kl, resp


@pytest.mark.parametrize("c", R.WIDTH_CASES, ids=repr)
def test_every_split_matches_float64(ops, c):
    """(D, P) with one column each, inside one slot, the private block at every position against the 64-lane slots and
    D + P = 256, raw heads on and off; D = 1: dtheta is exactly 0"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.EXPERT_CASES, ids=repr)
def test_every_expert_count_matches_float64(ops, c):
    """E = 1, 2, 3, 5, 8 at (8, 4) and both limits at once (E = 8, D + P = 256); E = 1: kl_mix is exactly 0, resp exactly 1"""
    _, _, resp = whole_op(ops, c)
    if c.E == 1:
        assert bool((resp == 1).all())


@pytest.mark.parametrize("c", R.ROW_CASES, ids=repr)
def test_every_row_count_matches_float64(ops, c):
    """one row, fewer rows than two workgroups' waves, 37 rows, and 1100 rows on 512 waves: a wave's second and third row"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.SPIKE_CASES + R.THETA0_CASES + R.TINY_CASES, ids=repr)
def test_saturated_softmax_zero_theta_and_tiny_scales_match_float64(ops, c):
    """`spike`: one raw-head row of expert 0 whose softmax saturates in a shared / in a private column (scale 1e-6 in every
    other column of BOTH blocks: the one softmax over W couples them); theta0: the prior N(0, 1) every model starts from;
    scales of 1e-5"""
    whole_op(ops, c)


@pytest.mark.parametrize("c", R.FAR_CASES, ids=repr)
def test_far_family_takes_the_saturated_path(ops, c):
    """independent shared means: every sample's own responsibility is 1 and kl_mix is log E"""
    _, kl, resp = whole_op(ops, c)
    own = torch.stack([resp[m, m] for m in range(c.E)])
    assert bool((own == 1).all()) and float((kl[:c.E].detach() - math.log(c.E)).abs().max()) <= 1e-6


def test_layout_of_the_decoder_batches(ops):
    """z[n] row block m: the shared columns are the same bits in every decoder's batch; the private columns are w_m in
    decoder m's own batch and aux_scale * eps_a[n][m], one float32 product, in every other"""
    c = R.FAMILY_CASES[0]
    inp, ref = reference(c)
    with torch.no_grad():
        z, _, _ = ops.mmplus_fusion(inp["theta"].to(DEV), [h.to(DEV) for h in inp["heads"]], inp["eps_u"].to(DEV),
                                    inp["eps_w"].to(DEV), inp["eps_a"].to(DEV), c.D, c.aux)
    E, B, D = c.E, c.B, c.D
    for n in range(E):
        assert torch.equal(z[n][:, :D], z[0][:, :D]), n
        for m in range(E):
            got = z[n][m * B:(m + 1) * B, D:]
            if n == m:
                assert R.rel_err(got, ref["z"][n][m * B:(m + 1) * B, D:]) <= R.TOL_Z
            else:
                assert torch.equal(got, torch.tensor(c.aux, device=DEV) * inp["eps_a"][n, m].to(DEV)), (n, m)


@pytest.mark.parametrize("c", R.FAMILY_CASES + [R.Case(2, 1, 1, R.B0, raw=True)], ids=repr)
def test_without_kl_gradient_the_backward_is_the_gather_of_dz(ops, c):
    """no dkl: dmu's shared columns ARE the sum over the decoders n, in order, of row block m of dz[n], its private columns
    row block m of dz[m] alone, and (heads that are not raw) dsigma is that times eps as one float32 product, bit for bit;
    dtheta is exactly 0"""
    inp, _ = reference(c)
    _, _, _, dheads, dtheta = run_op(ops, c, inp, use_kl=False)
    E, B, D = c.E, c.B, c.D
    gz = inp["gz"].to(DEV)
    for m in range(E):
        blocks = [gz[n][m * B:(m + 1) * B] for n in range(E)]
        gu = blocks[0][:, :D].clone()
        for n in range(1, E):
            gu = gu + blocks[n][:, :D]
        gw = blocks[m][:, D:]
        dmu, dsg = R.split_packed(dheads[m], c.W)
        assert torch.equal(dmu[:, :D], gu) and torch.equal(dmu[:, D:], gw), m
        if not c.raw:
            assert torch.equal(dsg[:, :D], gu * inp["eps_u"][m].to(DEV)), m
            assert torch.equal(dsg[:, D:], gw * inp["eps_w"][m].to(DEV)), m
    assert dtheta is not None and not bool(dtheta.any())


@pytest.mark.parametrize("c", R.FAMILY_CASES, ids=repr)
@pytest.mark.parametrize("use_kl,use_z", [(False, True), (True, False), (True, (0, 2)), (False, (1,))],
                         ids=["dkl-none", "dz-none", "dz1-none", "only-dz1"])
def test_absent_upstream_gradients(ops, c, use_kl, use_z):
    """dkl None, every dz None, ONE decoder's dz None, only one present: an absent gradient counts as zeros, not as stale
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
    if not use_kl and use_z is not True:      # only decoder 1's gradient: no other head's PRIVATE columns get anything
        for e in set(range(c.E)) - set(use_z):
            dmu, dsg = R.split_packed(dheads[e], c.W)
            assert not bool(dmu[:, c.D:].any()), e
            if not c.raw:
                assert not bool(dsg[:, c.D:].any()), e


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


@pytest.mark.parametrize("c", [R.Case(3, 32, 16, R.B0), R.Case(2, 192, 64, 7), R.Case(2, 65, 8, R.B0)], ids=repr)
def test_shared_rows_are_the_mixture_priors_and_private_rows_the_product_kernels(ops, c):
    """heads that are not raw: rows 0 .. 2E-1 and the shared columns of z against ops.mixprior_fusion on the contiguous
    shared slice; row 2E + m against ops.poe_reparam_kl(cols=(D, P)) on a zero theta: within TOL_KL / TOL_Z of each other"""
    inp, _ = reference(c)
    E, B, D, P, W = c.E, c.B, c.D, c.P, c.W
    theta = inp["theta"].to(DEV)
    heads = [h.to(DEV) for h in inp["heads"]]
    with torch.no_grad():
        z, kl, resp = ops.mmplus_fusion(theta, heads, inp["eps_u"].to(DEV), inp["eps_w"].to(DEV), inp["eps_a"].to(DEV), D, c.aux)
        shared = [torch.cat([h[:, :D], h[:, W:W + D]], -1).contiguous() for h in heads]
        z_mm, kl_mm, resp_mm = ops.mixprior_fusion(theta, shared, inp["eps_u"].to(DEV))
        assert R.rel_err(kl[:E], kl_mm[:E]) <= R.TOL_KL and R.rel_err(kl[E:2 * E], kl_mm[E:]) <= R.TOL_KL
        assert float((resp - resp_mm).abs().max()) <= R.TOL_RESP
        for m in range(E):
            assert R.rel_err(z[0][m * B:(m + 1) * B, :D], z_mm[m]) <= R.TOL_Z, m
            _, kl_p, z_p = ops.poe_reparam_kl(torch.zeros(1, P, device=DEV), [heads[m]], [inp["eps_w"][m].to(DEV)], 2, 0b10,
                                              cols=(D, P))
            assert R.rel_err(kl[2 * E + m], kl_p[1]) <= R.TOL_KL, m
            assert R.rel_err(z[m][m * B:(m + 1) * B, D:], z_p[0]) <= R.TOL_Z, m


# ---------------------------------------------------------------------------------------------
# refusals: return codes of the host entries; nothing is launched
# ---------------------------------------------------------------------------------------------
def _entries(hip_lib, H, E, D, P, aux=1.0):
    """-> (forward's return code, backward's, whether anything was written) for buffers that would hold the call"""
    B = 3
    n = max(min(E, H.MAX_EXPERTS), 1)
    W = max(D + P, 1)
    heads = torch.full((n, B, 2 * W), 0.25, device=DEV)
    dheads = torch.full_like(heads, 0.5)
    zs = torch.full((2, n, n * B, W), 0.5, device=DEV)              # z, dz
    eps = torch.full((n * n + 2 * n, B, W), 0.5, device=DEV)
    theta = torch.zeros(1, max(D, 1), device=DEV)
    kl = torch.full((3 * max(E, 1), B), 0.5, device=DEV)
    resp = torch.full((max(E, 1), max(E, 1), B), 0.5, device=DEV)
    dtheta = torch.full((1, max(D, 1)), 0.5, device=DEV)
    ws = torch.full((4 * max(D, 1),), 0.5, device=DEV)
    fa, ba = H.MmPlusFwdArgs(), H.MmPlusBwdArgs()
    for e in range(n):
        fa.mu[e] = ba.mu[e] = heads[e].data_ptr()
        fa.lv[e] = ba.lv[e] = heads[e].data_ptr() + 4 * W
        fa.z[e] = zs[0, e].data_ptr()
        ba.dz[e] = zs[1, e].data_ptr()
        ba.dmu[e] = dheads[e].data_ptr()
        ba.dlv[e] = dheads[e].data_ptr() + 4 * W
    rf = hip_lib.mmvae_mmplus_fwd(ctypes.byref(fa), H.ptr(theta), H.ptr(eps), H.ptr(eps), H.ptr(eps), aux, H.ptr(kl),
                                  H.ptr(resp), E, B, D, P, 2 * W, 0, H.stream())
    rb = hip_lib.mmvae_mmplus_bwd(ctypes.byref(ba), H.ptr(theta), H.ptr(eps), H.ptr(eps), H.ptr(resp), H.ptr(kl),
                                  H.ptr(dtheta), H.ptr(ws), E, B, D, P, 2 * W, 0, 0, H.stream())
    torch.cuda.synchronize()
    written = any(bool((t != 0.5).any()) for t in (zs, dheads, kl, resp, dtheta, ws))
    return rf, rb, written, int(hip_lib.mmvae_mmplus_ws_floats(B, D, P))


def test_refusals(hip_lib, ops):
    from multimodal_vae_comparison_amd import hipops as H
    U = H.ERR_UNSUPPORTED
    assert _entries(hip_lib, H, E=9, D=8, P=4) == (U, U, False, 8)      # (the workspace size does not depend on E)
    assert _entries(hip_lib, H, E=2, D=193, P=64) == (U, U, False, 0)
    assert _entries(hip_lib, H, E=2, D=8, P=0) == (U, U, False, 0)
    assert _entries(hip_lib, H, E=2, D=0, P=8) == (U, U, False, 0)
    assert _entries(hip_lib, H, E=0, D=8, P=4)[:3] == (U, U, False)
    # aux_scale is the forward pass's alone: zero, negative, infinite, NaN
    for aux in (0.0, -1.0, float("inf"), float("nan")):
        rf, _, _, _ = _entries(hip_lib, H, E=2, D=8, P=4, aux=aux)
        assert rf == H.ERR_ARG, aux
    heads = torch.full((2, 3, 24), 0.25, device=DEV)
    zs = torch.full((2, 6, 12), 0.5, device=DEV)
    fa = H.MmPlusFwdArgs()
    for e in range(2):
        fa.mu[e], fa.lv[e], fa.z[e] = heads[e].data_ptr(), heads[e].data_ptr() + 48, zs[e].data_ptr()
    eps, kl, resp = torch.zeros(8, 3, 12, device=DEV), torch.full((6, 3), 0.5, device=DEV), torch.full((2, 2, 3), 0.5, device=DEV)
    rf = hip_lib.mmvae_mmplus_fwd(ctypes.byref(fa), H.ptr(torch.zeros(1, 8, device=DEV)), H.ptr(eps), H.ptr(eps), H.ptr(eps),
                                  0.0, H.ptr(kl), H.ptr(resp), 2, 3, 8, 4, 24, 0, H.stream())
    torch.cuda.synchronize()
    assert rf == H.ERR_ARG and not any(bool((t != 0.5).any()) for t in (zs, kl, resp))
    # the same calls with nothing wrong with them are accepted, at both limits too
    assert _entries(hip_lib, H, E=2, D=8, P=4) == (0, 0, True, 8)
    assert _entries(hip_lib, H, E=8, D=192, P=64) == (0, 0, True, 192)
    # ... and the wrapper names what is wrong in its own words, or turns the library's refusal into an error
    th = torch.zeros(1, 8, device=DEV)
    good = dict(theta=th, packed=[torch.rand(3, 24, device=DEV) for _ in range(2)], eps_u=torch.randn(2, 3, 8, device=DEV),
                eps_w=torch.randn(2, 3, 4, device=DEV), eps_a=torch.randn(2, 2, 3, 4, device=DEV), D=8, aux_scale=1.0)
    for bad, match in ((dict(aux_scale=0.0), "aux_scale"), (dict(aux_scale=-2.0), "aux_scale"),
                       (dict(aux_scale=float("nan")), "aux_scale"), (dict(D=12), "P = 0"),
                       (dict(eps_u=torch.randn(2, 3, 4, device=DEV)), "eps_u"), (dict(eps_w=torch.randn(2, 3, 8, device=DEV)), "eps_w"),
                       (dict(eps_a=torch.randn(2, 3, 4, device=DEV)), "eps_a"), (dict(theta=torch.zeros(1, 12, device=DEV)), "theta"),
                       (dict(packed=[torch.rand(3, 24, device=DEV), torch.rand(3, 26, device=DEV)]), "heads")):
        with pytest.raises(ValueError, match=f"mmplus_fusion: .*{match}"):
            ops.mmplus_fusion(**dict(good, **bad))
    for E, D, P in ((9, 8, 4), (2, 193, 64)):
        with pytest.raises(RuntimeError, match="mmvae_mmplus_fwd failed: unsupported shape"):
            ops.mmplus_fusion(torch.zeros(1, D, device=DEV), [torch.rand(3, 2 * (D + P), device=DEV) for _ in range(E)],
                              torch.randn(E, 3, D, device=DEV), torch.randn(E, 3, P, device=DEV),
                              torch.randn(E, E, 3, P, device=DEV), D, 1.0)
