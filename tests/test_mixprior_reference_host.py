"""The float64 restatement of the mixture-of-experts prior (tests/mixprior_reference.py) against torch's own operations on
the CPU, so that tests/test_mixprior_fusion_gpu.py does not measure the kernel against a mistake: the mixture density and
the closed-form KL against torch.distributions, the properties of the estimate, the restatement in float32 against
float64 in BOTH arithmetic forms (why the kernel is written in the difference form), the overlap of the tests' inputs --
and the host side of the MMVM mixer: registry, `alpha`, its refusals, the loss weights.  Nothing here reaches a kernel.

Float32 against float64 on the CPU, inputs rounded to float32 first, worst over every case of the GPU suite (printed with
-s).  Difference form: z 6.0e-8, kl_mix rows 1.8e-6 of their maximum, every kl_mix entry 3.7e-6 over max(1, |entry|),
kl_std 2.2e-7, resp 1.5e-6 absolute, dmu 1.3e-6, dsigma 1.1e-6, du 4.9e-6, dtheta 4.7e-7: at least 5 x under the GPU bounds
(1e-5, 2e-5, 2e-5, 1e-5 absolute, 5e-5).  Plain form (absolute log-densities, then their logsumexp), kl_mix entries: 1.4e-4
at E = 8, D = 256 with raw heads (bound 2e-5) and 5.0e-3 / 5.6e-3 at scales of 1e-5 (E = 2, D = 32 / E = 8, D = 256), with
gradients 5.0e-3 / 7.0e-3 of their maximum there -- outside the bounds, where the difference form gives 3.2e-6, 3.4e-7 and
2.2e-6."""
import math

import pytest
import torch
import torch.distributions as dist
import torch.nn.functional as F

import mixprior_reference as R

F64 = torch.float64


def _inputs(c):
    inp = R.make_inputs(c)
    return [h.double() for h in inp["heads"]], inp["eps"].double(), inp["theta"].double()


@pytest.mark.parametrize("c", [R.Case(1, 1, 6), R.Case(2, 9, 6), R.Case(3, 70, 6, raw=True), R.Case(5, 8, 6, far=True),
                               R.Case(8, 256, 6, raw=True), R.Case(8, 256, 6, scale=R.TINY)], ids=repr)
def test_restatement_is_torch_distributions(c):
    """kl_mix = log q_m(z_m) - log h(z_m) with h a MixtureSameFamily over the E experts, kl_std = kl_divergence to the
    prior, resp from the component log-densities: 1e-10 in float64, both arithmetic forms"""
    heads, eps, theta = _inputs(c)
    mus, sgs = R.experts(heads, c.raw)
    comp = dist.Independent(dist.Normal(torch.stack(mus, 1), torch.stack(sgs, 1)), 1)         # batch (B, E), event D
    h = dist.MixtureSameFamily(dist.Categorical(probs=torch.full((c.B, c.E), 1.0 / c.E, dtype=F64)), comp)
    sp = (F.softmax(theta, -1) * c.D).expand(c.B, c.D)
    for form in R.FORMS:
        z, kl, resp = R.mixprior_reference(theta, heads, eps, c.raw, form)
        for m in range(c.E):
            assert torch.equal(z[m], mus[m] + sgs[m] * eps[m])
            qm = dist.Independent(dist.Normal(mus[m], sgs[m]), 1)
            want = qm.log_prob(z[m]) - h.log_prob(z[m])
            assert float((kl[m] - want).abs().max()) <= 1e-10, (form, m)
            std = dist.kl_divergence(dist.Normal(mus[m], sgs[m]), dist.Normal(torch.zeros_like(sp), sp)).sum(-1)
            assert float((kl[c.E + m] - std).abs().max()) <= 1e-10, (form, m)
            comp_lp = comp.log_prob(z[m].unsqueeze(1))                                        # (B, E)
            assert float((resp[m] - F.softmax(comp_lp, 1).T).abs().max()) <= 1e-10, (form, m)


@pytest.mark.parametrize("c", R.FAMILY_CASES + R.FAR_CASES + [R.Case(8, 8, R.B0), R.Case(2, 1, R.B0, raw=True)], ids=repr)
def test_properties_of_the_estimate(c):
    """kl_mix <= log E everywhere (h >= q_m / E); the responsibilities of a sample sum to 1 and its own is
    exp(kl_mix) / E; identical experts give 0"""
    heads, eps, theta = _inputs(c)
    _, kl, resp = R.mixprior_reference(theta, heads, eps, c.raw)
    assert bool((kl[:c.E] <= math.log(c.E)).all())
    assert float((resp.sum(1) - 1).abs().max()) <= 1e-12
    own = torch.stack([resp[m, m] for m in range(c.E)])
    assert float((own - kl[:c.E].exp() / c.E).abs().max()) <= 1e-12
    same = [heads[0].clone() for _ in range(c.E)]
    _, kl, resp = R.mixprior_reference(theta, same, eps, c.raw)
    assert float(kl[:c.E].abs().max()) <= 1e-12 and float((resp - 1.0 / c.E).abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype", [F64, torch.float32])
@pytest.mark.parametrize("raw", [False, True])
def test_one_expert_gives_exactly_zero(dtype, raw):
    c = R.Case(1, 8, 5, raw=raw)
    inp = R.make_inputs(c)
    _, kl, resp = R.mixprior_reference(inp["theta"].to(dtype), [inp["heads"][0].to(dtype)], inp["eps"].to(dtype), raw)
    assert not bool(kl[0].any()) and bool((resp == 1).all()) and bool(kl[1].all())


def test_the_estimate_is_unbiased_for_the_kl_to_the_mixture():
    """D = 1, E = 2: the mean of kl_mix[m] over 20 000 seeded draws lies within 4 standard errors of KL(q_m || h) by
    quadrature"""
    n = 20000
    mu, sg = torch.tensor([0.3, -0.4], dtype=F64), torch.tensor([0.6, 0.9], dtype=F64)
    heads = [torch.stack([mu[e], sg[e]]).expand(n, 2) for e in range(2)]
    eps = torch.randn(2, n, 1, generator=torch.Generator().manual_seed(12), dtype=F64)
    _, kl, _ = R.mixprior_reference(torch.zeros(1, 1, dtype=F64), heads, eps)
    x = torch.linspace(-12.0, 12.0, 200001, dtype=F64)
    lq = torch.stack([dist.Normal(mu[e], sg[e]).log_prob(x) for e in range(2)])
    lh = torch.logsumexp(lq, 0) - math.log(2)
    for m in range(2):
        want = float(torch.trapezoid(lq[m].exp() * (lq[m] - lh), x))
        mean, se = float(kl[m].mean()), float(kl[m].std()) / math.sqrt(n)
        print(f"KL(q_{m} || h): quadrature {want:.6f}, one-sample mean {mean:.6f} +- {se:.6f}")
        assert 0 < want < math.log(2) and abs(mean - want) <= 4 * se, (m, want, mean, se)


@pytest.mark.parametrize("raw", [False, True])
def test_autograd_matches_finite_differences(raw):
    c = R.Case(3, 3, 3, raw=raw)
    inp = R.make_inputs(c)
    heads = [h.double().requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].double().requires_grad_(True)
    eps = inp["eps"].double()
    for form in R.FORMS:
        def f(theta, *heads):
            z, kl, _ = R.mixprior_reference(theta, list(heads), eps, raw, form)
            return z, kl
        assert torch.autograd.gradcheck(f, (theta, *heads), eps=1e-7, atol=1e-6, rtol=1e-5)


def _all_cases():
    seen, out = set(), []
    for c in (R.WIDTH_CASES + R.EXPERT_CASES + R.ROW_CASES + R.SPIKE_CASES + R.THETA0_CASES + R.FAR_CASES + R.TINY_CASES
              + R.FAMILY_CASES + R.THETA_CASES):
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out


def _f32_against_f64(c, form, worst):
    inp = R.make_inputs(c)
    lo, hi = R.run_reference(c, inp, torch.float32, form=form), R.run_reference(c, inp)
    p = R.Parts(f"{c.name} [{form}]", worst)
    R.check_forward(p, c, lo["z"], lo["kl"], lo["resp"], hi)
    R.check_backward(p, c, lo["dheads"], lo["dtheta"], hi)
    return p


def test_difference_form_in_float32_stays_inside_the_gpu_bounds():
    """where the kernel's arithmetic comes from: the restatement in the difference form, evaluated in float32 on the CPU,
    against float64 over every case of the GPU suite -- each part inside the bound the device is held to, with a margin of 4"""
    worst = {}
    for c in _all_cases():
        _f32_against_f64(c, "difference", worst).done()
    print("difference form, float32 against float64, worst per part: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    bound = {"z": R.TOL_Z, "kl_mix": R.TOL_KL, "kl_std": R.TOL_KL, "kl_mix entry": R.TOL_KL, "resp": R.TOL_RESP}
    assert all(4 * v <= bound.get(k, R.TOL_GRAD) for k, v in worst.items()), worst


@pytest.mark.parametrize("c", [R.Case(8, 256, 7, raw=True)] + R.TINY_CASES, ids=repr)
def test_plain_form_in_float32_does_not(c):
    """the absolute log-densities reach the hundreds at D = 256 and log sigma -11.5 per column at scales of 1e-5: their
    logsumexp and the subtraction keep that rounding.  Measured here (kl_mix entries over max(1, |entry|)): E8-D256-B7-raw
    1.4e-4, E2-D32-B37-scale1e-05 5.0e-3, E8-D256-B7-scale1e-05 5.6e-3, against 3.2e-6, 3.4e-7 and 2.2e-6 in the
    difference form"""
    err = {}
    for form in R.FORMS:
        worst = {}
        _f32_against_f64(c, form, worst)
        err[form] = worst["kl_mix entry"]
    print(f"{c.name}: kl_mix entries, float32 against float64: difference {err['difference']:.2e}, plain {err['plain']:.2e}")
    assert err["difference"] <= R.TOL_KL / 4 < R.TOL_KL < err["plain"], err


def test_inputs_overlap_and_case_tables():
    """at least half of the (m, b) rows keep their largest responsibility below 0.9 for E = 2 .. 8 and D = 8 .. 256 (the
    condition run_reference asserts); the far family saturates"""
    for E in (2, 3, 5, 8):
        for D in (8, 32, 70, 256):
            for raw in (False, True):
                c = R.Case(E, D, R.B0, raw=raw)
                assert c.overlaps
                frac = R.overlap_fraction(R.run_reference(c, R.make_inputs(c))["resp"])
                print(f"{c.name}: {frac:.2f} of the rows overlap")
                assert frac >= 0.5, (c.name, frac)
    for c in R.FAR_CASES:
        ref = R.run_reference(c, R.make_inputs(c))
        assert R.overlap_fraction(ref["resp"]) == 0.0 and not c.overlaps
        assert float((ref["kl"][:c.E] - math.log(c.E)).abs().max()) <= 1e-12
    assert R.spread(1) == R.spread(4) == 0.3 and R.spread(256) == pytest.approx(0.0375)
    names = {c.name for c in _all_cases()}
    assert {(c.D, c.raw) for c in R.WIDTH_CASES} == {(D, raw) for D in (1, 8, 63, 64, 65, 256) for raw in (False, True)}
    assert {c.E for c in R.EXPERT_CASES if c.D == 8} == {1, 2, 3, 5, 8} and "E8-D256-B7" in names and "E8-D256-B7-raw" in names
    assert {c.B for c in R.ROW_CASES} == {1, 5, 37, 1100} and R.B0 == 37
    assert all(c.spike and c.raw for c in R.SPIKE_CASES) and all(c.theta0 for c in R.THETA0_CASES)
    a, b = R.make_inputs(R.FAMILY_CASES[0]), R.make_inputs(R.FAMILY_CASES[0])
    assert all(torch.equal(x, y) for x, y in zip(a["heads"] + [a["eps"], a["gz"]], b["heads"] + [b["eps"], b["gz"]]))
    # the spike row: expert 0's scale is 1e-6 (+ e^-40) in every column but one
    inp = R.make_inputs(R.SPIKE_CASES[0])
    sg = R.experts(inp["heads"], True)[1][0][3]
    assert int((sg < 1.1e-6).sum()) == 31 and float(sg.max()) > 0.99
    # the launch geometry is the other fusions': one partial prior-gradient row per workgroup of four waves
    from multimodal_vae_comparison_amd import hipops
    L = hipops.lib()
    assert L.mmvae_mixprior_ws_floats(1100, 32) == (R.MAX_WAVES // 4) * 32 and 1100 > 2 * R.MAX_WAVES
    assert L.mmvae_mixprior_ws_floats(5, 70) == 2 * 70 and L.mmvae_mixprior_ws_floats(1, 1) == 1
    assert L.mmvae_mixprior_ws_floats(5, 257) == 0 and L.mmvae_mixprior_ws_floats(0, 8) == 0


def test_wrapper_checks_the_noise_shape_on_the_host():
    from multimodal_vae_comparison_amd import ops
    heads = [torch.zeros(3, 8) for _ in range(2)]
    with pytest.raises(ValueError, match=r"eps is \(3, 4\)"):
        ops.mixprior_fusion(torch.zeros(1, 4), heads, torch.zeros(3, 4))


def test_mixprior_is_in_the_makefile():
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "Makefile")).read()
    srcs = next(line for line in src.splitlines() if line.startswith("SRCS"))
    assert "mixprior.hip" in srcs.split()
    assert os.path.exists(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "mixprior.hip"))


# ---------------------------------------------------------------------------------------------
# the mixer's host side
# ---------------------------------------------------------------------------------------------
def _trainer(mods=None, model_cfg=None, **kw):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods("mmvm", CD_MODS if mods is None else mods, 8, batch_size=4, **kw)
    if model_cfg is not None:
        cfg["model_cfg"] = model_cfg
    return MultimodalVAE(cfg, feature_dims=dims, device="cpu")


def test_registry_alpha_and_loss_weights():
    from multimodal_vae_comparison_amd import models
    from multimodal_vae_comparison_amd.models.mmvae_models import MMVM, MOE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, step_flops_per_sample
    assert models.mmvm is MMVM and "mmvm" in models.__all__ and issubclass(MMVM, MOE)
    model = _trainer().model
    assert isinstance(model, MMVM) and model.modelName == "mmvm" and model.alpha == 1.0      # the paper's objective
    assert _trainer(model_cfg={}).model.alpha == 1.0
    assert _trainer(model_cfg={"alpha": 0.25}).model.alpha == 0.25
    assert _trainer(model_cfg={"alpha": 0}).model.alpha == 0.0 and _trainer(model_cfg={"alpha": 1}).model.alpha == 1.0
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            _trainer(model_cfg={"alpha": bad})
    # the loss weights over [2 recon rows, 2 kl_mix rows, 2 kl_std rows]: llik, beta alpha, beta (1 - alpha)
    mods = [dict(m, llik_scaling=s) for m, s in zip(CD_MODS, (1.0, 2.0))]
    W = _trainer(mods=mods, model_cfg={"alpha": 0.25}, beta=2.0).model._mm_weights()
    assert W[0] == pytest.approx([1.0, 2.0, 0.5, 0.5, 1.5, 1.5]) and W[1] == pytest.approx([0, 0, 0.25, 0.25, 0.75, 0.75])
    assert W[2] == [0, 0, 1, 1, 0, 0] and W[3] == [0, 0, 0, 0, 1, 1]
    W = _trainer(beta=2.5).model._mm_weights()      # alpha = 1: the fixed prior's rows carry exactly 0
    assert W[0] == [1.0, 1.0, 2.5, 2.5, 0.0, 0.0]
    # inference and the evaluation hooks are MOE's own
    for name in ("forward", "_sample", "_proposal", "_unimodal", "_proposal_size", "modality_mixing"):
        assert getattr(MMVM, name) is getattr(MOE, name), name
    # one encoder and one decoder pass per modality in the FLOP count (moe: M decoder passes)
    meta = {"mixing": "mmvm", "mods": CD_MODS, "D": 16, "T": 32}
    assert step_flops_per_sample(meta) == step_flops_per_sample(dict(meta, mixing="mmjsd"))
    assert step_flops_per_sample(meta) < step_flops_per_sample(dict(meta, mixing="moe"))


def test_refusals_name_their_cause():
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch
    with pytest.raises(NotImplementedError, match="mmvm: private_latents"):
        _trainer(mods=[dict(m, private=4) for m in CD_MODS])
    with pytest.raises(NotImplementedError, match="mmvm: obj 'iwae'"):
        _trainer(obj="iwae")
    with pytest.raises(NotImplementedError, match="mmvm: obj 'dreg'"):
        _trainer(obj="dreg")
    with pytest.raises(NotImplementedError, match="mmvm: K = 4"):
        _trainer(K=4)
    with pytest.raises(NotImplementedError, match="mmvm: prior 'laplace'"):
        _trainer(prior="laplace")
    model = _trainer().model
    batch = cdsprites_batch(4, 6, seed=3)
    batch["mod_2"] = dict(batch["mod_2"], data=None)
    with pytest.raises(ValueError, match=r"mmvm.*mod_2.*every modality"):
        model.objective(batch)
