"""The float64 restatement tests/test_mmplus_fusion_gpu.py holds the kernels to (tests/mmplus_reference.py), pinned to
torch.distributions on the CPU: kl_mix to Normal.log_prob + logsumexp, kl_u and kl_w to kl_divergence, the difference form
to the plain form; one expert (the mixture is the expert; kl_u + kl_w is the KL of the W-wide Gaussian against [sp | 1]);
the layout of the decoder batches and which gradient reaches which head column; the overlap condition of every case.
Nothing here reaches a kernel."""
import math

import pytest
import torch
import torch.distributions as dist
import torch.nn.functional as F

import mmplus_reference as R

F64 = torch.float64
CASES = [R.Case(3, 8, 4, 11), R.Case(3, 8, 4, 11, raw=True), R.Case(2, 60, 10, 9, raw=True), R.Case(2, 1, 1, 9),
         R.Case(3, 32, 16, 9, far=True)]


def _inputs(c):
    inp = R.make_inputs(c)
    return inp, [h.to(F64) for h in inp["heads"]], inp["theta"].to(F64), [inp[k].to(F64) for k in ("eps_u", "eps_w", "eps_a")]


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_restatement_against_torch_distributions(c):
    inp, heads, theta, (eu, ew, ea) = _inputs(c)
    z, kl, resp = R.mmplus_reference(theta, heads, eu, ew, ea, c.D, c.aux, c.raw)
    E, B, D, W = c.E, c.B, c.D, c.W
    mus, sgs = R.posteriors(heads, c.raw)
    sp = F.softmax(theta, 1) * D
    for m in range(E):
        qu = [dist.Normal(mus[j][:, :D], sgs[j][:, :D]) for j in range(E)]
        u = z[0][m * B:(m + 1) * B, :D]
        assert torch.allclose(u, mus[m][:, :D] + sgs[m][:, :D] * eu[m], rtol=0, atol=1e-14)
        lq = torch.stack([q.log_prob(u).sum(-1) for q in qu])
        want = lq[m] - (torch.logsumexp(lq, 0) - math.log(E))
        assert float((kl[m] - want).abs().max()) <= 1e-9 * max(1.0, float(lq.abs().max())), m
        assert float((resp[m] - F.softmax(lq, 0)).abs().max()) <= 1e-10, m
        want_u = dist.kl_divergence(qu[m], dist.Normal(torch.zeros_like(sp), sp)).sum(-1)
        assert torch.allclose(kl[E + m], want_u, rtol=1e-12, atol=1e-12), m
        qw = dist.Normal(mus[m][:, D:], sgs[m][:, D:])
        want_w = dist.kl_divergence(qw, dist.Normal(torch.zeros(()).to(F64), torch.ones(()).to(F64))).sum(-1)
        assert torch.allclose(kl[2 * E + m], want_w, rtol=1e-12, atol=1e-12), m
    # the difference form is the plain form
    z2, kl2, resp2 = R.mmplus_reference(theta, heads, eu, ew, ea, c.D, c.aux, c.raw, form="plain")
    assert float((kl - kl2).abs().max()) <= 1e-9 * max(1.0, float(kl2.abs().max()))
    assert float((resp - resp2).abs().max()) <= 1e-10 and all(torch.equal(a, b) for a, b in zip(z, z2))


@pytest.mark.parametrize("raw", [False, True], ids=["lv", "raw"])
def test_one_expert(raw):
    """E = 1: kl_mix is identically 0, resp 1, and kl_u + kl_w is the KL of the W-wide Gaussian against N(0, [sp | 1])"""
    c = R.Case(1, 8, 4, 11, raw=raw)
    inp, heads, theta, (eu, ew, ea) = _inputs(c)
    z, kl, resp = R.mmplus_reference(theta, heads, eu, ew, ea, c.D, c.aux, raw)
    assert not bool(kl[0].any()) and bool((resp == 1).all()) and tuple(z[0].shape) == (c.B, c.W)
    mus, sgs = R.posteriors(heads, raw)
    prior = torch.cat([F.softmax(theta, 1) * c.D, torch.ones(1, c.P, dtype=F64)], -1)
    want = dist.kl_divergence(dist.Normal(mus[0], sgs[0]), dist.Normal(torch.zeros_like(prior), prior)).sum(-1)
    assert torch.allclose(kl[1] + kl[2], want, rtol=1e-12, atol=1e-12)


def _none(g):
    """no gradient: absent, or exact zeros"""
    return g is None or not bool(g.any())


def test_layout_and_gradient_routing():
    """z[n] row block m is [u_m | w_m] for n == m and [u_m | s eps_a[n][m]] otherwise; eps_a and the off-diagonal private
    columns carry no gradient to any head; the shared columns of row block m reach head m from EVERY decoder's batch; with
    raw heads the one softmax over W couples the blocks: a gradient on shared columns alone reaches the private logits"""
    for raw in (False, True):
        c = R.Case(3, 8, 4, 5, raw=raw)
        inp, heads, theta, (eu, ew, ea) = _inputs(c)
        E, B, D, W = c.E, c.B, c.D, c.W
        heads = [h.requires_grad_(True) for h in heads]
        ea = ea.clone().requires_grad_(True)
        z, _, _ = R.mmplus_reference(theta, heads, eu, ew, ea, D, c.aux, raw)
        mus, sgs = R.posteriors(heads, raw)
        for n in range(E):
            assert tuple(z[n].shape) == (E * B, W)
            for m in range(E):
                blk = z[n][m * B:(m + 1) * B]
                assert torch.equal(blk[:, :D], (mus[m][:, :D] + sgs[m][:, :D] * eu[m]))
                if n == m:
                    assert torch.equal(blk[:, D:], mus[m][:, D:] + sgs[m][:, D:] * ew[m])
                else:
                    assert torch.equal(blk[:, D:], c.aux * ea[n, m])
        # the off-diagonal private columns: a function of eps_a alone
        off = sum(z[n][m * B:(m + 1) * B, D:].sum() for n in range(E) for m in range(E) if n != m)
        g = torch.autograd.grad(off, heads + [ea], allow_unused=True, retain_graph=True)
        assert all(_none(x) for x in g[:E])
        assert bool((g[E].diagonal(dim1=0, dim2=1) == 0).all()) and float(g[E][0, 1].min()) == c.aux      # the diagonal is never read
        # decoder 2's batch, row block 0, shared columns: head 0 only
        g = torch.autograd.grad(z[2][:B, :D].sum(), heads, allow_unused=True, retain_graph=True)
        assert _none(g[1]) and _none(g[2])
        dmu, dlv = R.split_packed(g[0], W)
        assert bool((dmu[:, :D] == 1).all()) and not bool(dmu[:, D:].any())
        if raw:
            assert bool(dlv[:, D:].any()), "raw heads: the softmax over W couples the private logits to a shared gradient"
            assert float(dlv.sum(-1).abs().max()) <= 1e-12      # (a softmax's gradient sums to 0 over its W columns)
        else:
            assert torch.equal(dlv[:, :D], eu[0]) and not bool(dlv[:, D:].any())
        # decoder 1's own private block: head 1's private columns only
        g = torch.autograd.grad(z[1][B:2 * B, D:].sum(), heads, allow_unused=True)
        assert _none(g[0]) and _none(g[2]) and bool(R.split_packed(g[1], W)[0][:, D:].all()) and not bool(R.split_packed(g[1], W)[0][:, :D].any())


def test_every_case_overlaps_where_it_must():
    """run_reference asserts the condition; here for every case table of the GPU file, on the reference alone"""
    seen, held = set(), 0
    for c in R.ALL_CASES:
        if c.name in seen or c.B > 200:      # (the 1100-row cases: the same recipe, checked by the GPU run's reference)
            continue
        seen.add(c.name)
        ref = R.run_reference(c, R.make_inputs(c))
        if c.overlaps:
            held += 1
            assert R.overlap_fraction(ref["resp"]) >= 0.5, c.name
        if c.far:
            assert R.overlap_fraction(ref["resp"]) == 0.0, c.name
    assert held >= 30


def test_restatement_in_float32_is_close_to_float64():
    """the tolerances of the GPU file leave room for float32 itself: the restatement evaluated in float32 on the CPU"""
    for c in R.FAMILY_CASES:
        inp = R.make_inputs(c)
        r64, r32 = R.run_reference(c, inp), R.run_reference(c, inp, dtype=torch.float32)
        p = R.Parts(c.name + " [float32 on the host]")
        R.check_forward(p, c, r32["z"], r32["kl"], r32["resp"], r64)
        R.check_backward(p, c, r32["dheads"], r32["dtheta"], r64)
        p.done()


def test_mmplus_is_in_the_makefile_and_the_header():
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "Makefile")).read()
    srcs = next(line for line in src.splitlines() if line.startswith("SRCS"))
    assert "mmplus.hip" in srcs.split()
    assert os.path.exists(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "mmplus.hip"))
    header = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    from multimodal_vae_comparison_amd import hipops as H
    for name in ("mmvae_mmplus_fwd", "mmvae_mmplus_bwd", "mmvae_mmplus_ws_floats"):
        assert name + "(" in header and name in H.SIGNATURES, name
