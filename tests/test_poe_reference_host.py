"""The float64 restatement of the product-of-experts fusion (tests/poe_reference.py) against torch's own operations on
the CPU, so that tests/test_poe_fusion_gpu.py does not measure the kernels against a mistake: KL rows against
torch.distributions, the joint against the product of Gaussians written element by element, the pass-through mode, raw
heads, column ranges, autograd against finite differences -- and the case tables against the dispatch they claim to cover."""
import math

import pytest
import torch
import torch.distributions as dist
import torch.nn.functional as F

import poe_reference as R

F64 = torch.float64


def _inputs(E, n_z, D, B, wp=1, raw=False, Dtot=None):
    c = R.Case("host", E, n_z, D, B, wp, (1 << (E + 1)) - 1, raw=raw, Dtot=Dtot if Dtot else D,
               cols=None if Dtot is None else (0, D))
    inp = R.make_inputs(c)
    return ([h.double() for h in inp["heads"]], [e.double() for e in inp["eps"]], inp["theta"].double())


@pytest.mark.parametrize("E,D,wp", [(1, 1, 1), (2, 9, 1), (3, 70, 0), (1, 20, 2), (8, 16, 1)])
def test_kl_rows_are_torch_distributions_kl(E, D, wp):
    heads, eps, theta = _inputs(E, 1, D, 6, wp)
    joint, kl, _ = R.poe_reference(theta, heads, eps, wp, (1 << (E + 1)) - 1)
    prior = dist.Normal(torch.zeros(1, D, dtype=F64), F.softmax(theta, -1) * D)
    for e, h in enumerate(heads):
        want = dist.kl_divergence(dist.Normal(h[:, :D], h[:, D:]), prior).sum(-1)
        assert torch.allclose(kl[e], want, rtol=1e-12, atol=1e-12), e
    want = dist.kl_divergence(dist.Normal(joint[0], joint[1]), prior).sum(-1)
    assert torch.allclose(kl[E], want, rtol=1e-12, atol=1e-12)


def test_rows_outside_the_mask_are_zero_and_the_others_unchanged():
    heads, eps, theta = _inputs(3, 1, 7, 5)
    full = R.poe_reference(theta, heads, eps, 1, 0b1111)[1]
    for mask in R.masks(3):
        kl = R.poe_reference(theta, heads, eps, 1, mask)[1]
        for j in range(4):
            assert torch.equal(kl[j], full[j] if mask >> j & 1 else torch.zeros(5, dtype=F64))
    assert R.masks(3) == [0, 0b0001, 0b1000, 0b0111, 0b1111]


@pytest.mark.parametrize("E,wp", [(1, 0), (1, 1), (3, 0), (3, 1), (8, 1)])
def test_joint_is_the_product_of_gaussians(E, wp):
    """precision-weighted mean over the experts (variance exp(lv) + 1e-8 each) and, with_prior, N(0, 1 + 1e-8), written
    element by element in Python floats; z = muJ + varJ eps"""
    B, D = 3, 5
    heads, eps, theta = _inputs(E, 2, D, B, wp)
    joint, _, z = R.poe_reference(theta, heads, eps, wp, 0)
    for b in range(B):
        for d in range(D):
            prec = [1.0 / (math.exp(float(h[b, D + d])) + 1e-8) for h in heads]
            mus = [float(h[b, d]) for h in heads]
            if wp:
                prec.append(1.0 / (1.0 + 1e-8))
                mus.append(0.0)
            var = 1.0 / sum(prec)
            mean = sum(m * p for m, p in zip(mus, prec)) * var
            assert math.isclose(float(joint[0, b, d]), mean, rel_tol=1e-12, abs_tol=1e-14)
            assert math.isclose(float(joint[1, b, d]), var, rel_tol=1e-12)
            for i in range(2):
                assert math.isclose(float(z[i, b, d]), mean + var * float(eps[i][b, d]), rel_tol=1e-12, abs_tol=1e-14)


def test_pass_through_returns_expert_0_untouched():
    heads, eps, theta = _inputs(1, 3, 20, 6, wp=2)
    joint, kl, z = R.poe_reference(theta, heads, eps, 2, 0b11)
    assert torch.equal(joint[0], heads[0][:, :20]) and torch.equal(joint[1], heads[0][:, 20:])
    assert torch.equal(kl[0], kl[1])
    for i in range(3):
        assert torch.equal(z[i], heads[0][:, :20] + heads[0][:, 20:] * eps[i])
    with pytest.raises(AssertionError):
        R.poe_reference(theta, heads * 2, eps, 2, 0)


@pytest.mark.parametrize("E,D,wp", [(2, 1, 1), (3, 33, 1), (1, 70, 0)])
def test_raw_is_the_softmaxed_head(E, D, wp):
    heads, eps, theta = _inputs(E, 2, D, 5, wp, raw=True)
    cooked = [torch.cat([h[:, :D], F.softmax(h[:, D:], -1) + 1e-6], -1) for h in heads]
    mask = (1 << (E + 1)) - 1
    for a, b in zip(R.poe_reference(theta, heads, eps, wp, mask, raw=True), R.poe_reference(theta, cooked, eps, wp, mask)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("col0,D,Dtot", [(0, 20, 30), (20, 10, 30), (70, 80, 150)])
@pytest.mark.parametrize("E,wp", [(2, 0), (1, 2)])
def test_cols_is_slicing_the_inputs_first(col0, D, Dtot, E, wp):
    heads, eps, theta = _inputs(E, 2, D, 4, wp, Dtot=Dtot)
    assert heads[0].shape == (4, 2 * Dtot) and theta.shape == (1, D)
    sliced = [torch.cat([h[:, col0:col0 + D], h[:, Dtot + col0:Dtot + col0 + D]], -1) for h in heads]
    mask = (1 << (E + 1)) - 1
    for a, b in zip(R.poe_reference(theta, heads, eps, wp, mask, cols=(col0, D)), R.poe_reference(theta, sliced, eps, wp, mask)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("E,wp,raw,cols", [(2, 1, False, None), (2, 0, True, None), (1, 2, False, None), (2, 0, False, (1, 2))])
def test_autograd_matches_finite_differences(E, wp, raw, cols):
    B, Dtot = 2, 3
    D = cols[1] if cols else Dtot
    g = torch.Generator().manual_seed(5)
    heads = []
    for _ in range(E):
        mu, u = torch.randn(B, Dtot, generator=g, dtype=F64), torch.randn(B, Dtot, generator=g, dtype=F64)
        lv = u if raw else (u.abs() * 0.5 + 0.1 if wp == 2 else F.softmax(u, -1) + 1e-6)
        heads.append(torch.cat([mu, lv], -1).requires_grad_(True))
    eps = [torch.randn(B, D, generator=g, dtype=F64) for _ in range(2)]
    theta = (torch.randn(1, D, generator=g, dtype=F64) * 0.3).requires_grad_(True)
    mask = (1 << (E + 1)) - 1

    def f(theta, *heads):
        _, kl, z = R.poe_reference(theta, list(heads), eps, wp, mask, cols=cols, raw=raw)
        return kl, z
    assert torch.autograd.gradcheck(f, (theta, *heads), eps=1e-7, atol=1e-6, rtol=1e-5)


def test_split_packed_and_rel_err():
    g = torch.arange(24.0).reshape(2, 12)
    a, b = R.split_packed(g, 6)
    assert torch.equal(a, g[:, :6]) and torch.equal(b, g[:, 6:])
    with pytest.raises(AssertionError):
        R.split_packed(g, 5)
    assert R.rel_err(torch.zeros(3), torch.zeros(3)) == 0.0
    assert R.rel_err(torch.tensor([1.0, 0.0]), torch.tensor([1.0, 1e-3])) == pytest.approx(1e-3)
    assert R.rel_err(torch.tensor([1e-9]), torch.zeros(1)) > 1.0          # nonzero against an all-zero reference fails
    assert not math.isfinite(R.rel_err(torch.tensor([float("nan")]), torch.ones(1)))
    p = R.Parts("x")
    p.check("fine", torch.tensor([1.0, 100.0]), torch.tensor([1.001, 100.0]), 5e-5)
    p.exact_zero("zeros", torch.zeros(4))
    p.done()
    p.check("small half", torch.tensor([1.0]), torch.tensor([1.001]), 5e-5)     # (passed above, beside the 100)
    p.exact_zero("not zero", torch.tensor([0.0, 1e-30]))
    with pytest.raises(AssertionError, match="small half.*not zero"):
        p.done()


def test_reference_in_float32_is_within_5e_7_of_float64():
    """where the tolerances of the GPU suite come from: the restatement evaluated in float32 on the CPU against float64,
    part by part, over cases spanning D = 1 .. 256, E = 1 .. 8, raw on and off and the three with_prior modes"""
    by_name = {c.name: c for c in R.FAST_CASES + R.GENERIC_CASES + R.RAW_CASES + R.PASS_THROUGH_CASES}
    names = ["E2-nz1-D1-B37-wp1-m111", "E2-nz1-D64-B37-wp1-m111", "E2-nz1-D256-B37-wp1-m111", "E8-nz8-D256-B7-wp1-m111111111",
             "E2-nz1-D32-B37-wp0-m111", "E2-nz1-D256-B37-wp1-m111-raw", "E3-nz3-D32-B37-wp1-m1111-raw",
             "E1-nz3-D70-B37-wp2-m10", "E2-nz2-D70-B37-wp1-m111-raw-spike"]
    worst = {}
    for n in names:
        c = by_name[n]
        inp = R.make_inputs(c)
        lo, hi = R.run_reference(c, inp, torch.float32), R.run_reference(c, inp)
        p = R.Parts(n, worst)
        R.check_forward(p, c, lo["joint"], lo["kl"], lo["z"], hi)
        R.check_backward(p, c, lo["dheads"], lo["dtheta"], hi)
        p.done()
    assert max(worst.values()) <= 5e-7, worst


# ---------------------------------------------------------------------------------------------
# the case tables cover what they say
# ---------------------------------------------------------------------------------------------
def test_case_tables_reach_every_dispatch_path():
    assert all(c.fast for c in R.FAST_CASES) and not any(c.fast for c in R.GENERIC_CASES)
    assert {c.D for c in R.FAST_CASES} >= {1, 20, 63, 64} and {c.D for c in R.GENERIC_CASES} >= {65, 128, 129, 192, 256}
    assert {(c.E, c.n_z) for c in R.FAST_CASES} >= {(1, 0), (1, 3), (3, 0), (3, 3)}
    assert {(c.E, c.n_z, c.D) for c in R.GENERIC_CASES} >= {(4, 1, 32), (8, 1, 16), (2, 4, 32), (1, 8, 8), (8, 8, 256)}
    for table in (R.FAST_CASES, R.GENERIC_CASES, R.RAW_CASES):
        assert {c.B for c in table} >= {513, 1100} and {c.with_prior for c in table} == {0, 1}
        assert {c.kl_mask for c in table if c.E == 3} >= set(R.masks(3))
        assert any(c.kl_mask == 0 and c.n_z > 0 for c in table)
    assert {c.B for c in R.FAST_CASES} >= {1, 5}
    assert all(c.raw for c in R.RAW_CASES) and {c.D for c in R.RAW_CASES} >= {1, 64, 65, 256}
    assert {c.E for c in R.RAW_CASES} >= {1, 3, 4} and {c.fast for c in R.RAW_CASES if c.spike} == {True, False}
    assert all(c.with_prior == 2 and c.E == 1 for c in R.PASS_THROUGH_CASES)
    assert {(c.D, c.n_z, c.kl_mask) for c in R.PASS_THROUGH_CASES} >= {(D, n, m) for D in (20, 70) for n in (1, 3) for m in (0, 2)}
    assert any(c.n_z == 4 and c.D <= 64 for c in R.PASS_THROUGH_CASES) and any(c.theta0 for c in R.PASS_THROUGH_CASES)
    assert {(c.Dtot, c.cols) for c in R.COLUMN_CASES} == {(30, (0, 20)), (30, (20, 10)), (150, (0, 70)), (150, (70, 80))}
    assert [c.fast for c in R.FAMILY_CASES] == [True, False] and {c.fast for c in R.THETA_CASES} == {True, False}
    assert {c.B for c in R.THETA_CASES} == {5, 1100}
    assert 1100 > 2 * R.MAX_WAVES and 513 == R.MAX_WAVES + 1


def test_inputs_hold_the_edges_the_gpu_tests_rely_on():
    spike = next(c for c in R.RAW_CASES if c.spike and c.fast)
    inp = R.make_inputs(spike)
    lv = F.softmax(inp["heads"][0][:, spike.Dtot:], -1) + 1e-6
    assert float(lv[3].max()) == pytest.approx(1.0, abs=1e-5) and float(lv[3].min()) == pytest.approx(1e-6, rel=1e-5)
    assert float(lv[2].min()) > 1e-4                               # (the other rows are ordinary)
    assert not R.make_inputs(next(c for c in R.PASS_THROUGH_CASES if c.theta0))["theta"].any()
    wp2 = R.make_inputs(R.PASS_THROUGH_CASES[0])["heads"][0]
    assert float(wp2[:, 20:].min()) >= 0.1
    a, b = R.make_inputs(R.FAST_CASES[0]), R.make_inputs(R.FAST_CASES[0])
    assert all(torch.equal(x, y) for x, y in zip(a["heads"], b["heads"])) and torch.equal(a["gkl"], b["gkl"])
    d1 = R.run_reference(R.FAST_CASES[0], a)                       # D = 1: the prior cannot move
    assert R.FAST_CASES[0].D == 1 and not d1["dtheta"].any()
