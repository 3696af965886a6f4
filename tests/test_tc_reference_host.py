"""The float64 restatement of the total-correlation fusion (tests/tc_reference.py) against torch's own operations on the
CPU, so that tests/test_tc_fusion_gpu.py does not measure the kernel against a mistake: every KL row against
torch.distributions, autograd against finite differences, the restatement in float32 against float64 (where the GPU
suite's tolerances come from), the case tables against the launch geometry -- and the host side of the MVTCAE mixer:
registry, `alpha`, its refusals, and the joint of forward() with one modality given.  Nothing here reaches a kernel."""
import math

import pytest
import torch
import torch.distributions as dist
import torch.nn.functional as F

import poe_reference as PR
import tc_reference as R

F64 = torch.float64


def _inputs(E, D, B, raw=False):
    inp = R.make_inputs(R.Case(E, D, B, raw=raw))
    return [h.double() for h in inp["heads"]], inp["eps"].double(), inp["theta"].double()


@pytest.mark.parametrize("E,D,raw", [(1, 1, False), (2, 9, False), (3, 70, True), (5, 8, False), (8, 16, True)])
def test_kl_rows_are_torch_distributions_kl(E, D, raw):
    heads, eps, theta = _inputs(E, D, 6, raw)
    joint, kl, z = R.tc_reference(theta, heads, eps, raw)
    q = dist.Normal(joint[0], joint[1])
    for e, h in enumerate(heads):
        lv = (F.softmax(h[:, D:], -1) + 1e-6) if raw else h[:, D:]
        want = dist.kl_divergence(q, dist.Normal(h[:, :D], torch.exp(lv) + 1e-8)).sum(-1)      # sigma_e = 1 / T_e
        assert float((kl[e] - want).abs().max()) <= 1e-9, e
    prior = dist.Normal(torch.zeros(1, D, dtype=F64), F.softmax(theta, -1) * D)
    assert float((kl[E] - dist.kl_divergence(q, prior).sum(-1)).abs().max()) <= 1e-9
    assert torch.equal(z, joint[0] + joint[1] * eps)


@pytest.mark.parametrize("E", [1, 3])
def test_joint_is_the_product_without_a_prior_expert(E):
    """the joint and z are those of the product-of-experts restatement with with_prior = 0, the prior row its row E"""
    heads, eps, theta = _inputs(E, 7, 5)
    joint, kl, z = R.tc_reference(theta, heads, eps)
    pj, pkl, pz = PR.poe_reference(theta, heads, [eps], 0, 1 << E)
    assert torch.equal(joint, pj) and torch.equal(z, pz[0]) and torch.equal(kl[E], pkl[E])
    if E == 1:      # the product of one expert is that expert: mean mu_0, "variance" exp(lv_0) + 1e-8
        assert torch.allclose(joint[0], heads[0][:, :7], rtol=1e-14, atol=0)
        assert torch.allclose(joint[1], torch.exp(heads[0][:, 7:]) + 1e-8, rtol=1e-14, atol=0)
        assert float(kl[0].abs().max()) < 1e-13


@pytest.mark.parametrize("E,raw", [(1, False), (2, True), (3, False)])
def test_autograd_matches_finite_differences(E, raw):
    B, D = 2, 3
    g = torch.Generator().manual_seed(5)
    heads = []
    for _ in range(E):
        mu, u = torch.randn(B, D, generator=g, dtype=F64), torch.randn(B, D, generator=g, dtype=F64)
        heads.append(torch.cat([mu, u if raw else F.softmax(u, -1) + 1e-6], -1).requires_grad_(True))
    eps = torch.randn(B, D, generator=g, dtype=F64)
    theta = (torch.randn(1, D, generator=g, dtype=F64) * 0.3).requires_grad_(True)

    def f(theta, *heads):
        _, kl, z = R.tc_reference(theta, list(heads), eps, raw)
        return kl, z
    assert torch.autograd.gradcheck(f, (theta, *heads), eps=1e-7, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("E", R.EXPERTS)
def test_reference_in_float32_is_within_2e_6_of_float64(E):
    """where the tolerances of the GPU suite come from: the restatement evaluated in float32 on the CPU against float64,
    part by part, each on its own float64 maximum (the expert row of ONE expert, analytically 0: on the prior row's), over
    D = 1 .. 256, B = 1 .. 130, raw on and off"""
    worst = {}
    for D in R.WIDTHS:
        for B in (1, 5, 130):
            for raw in (False, True):
                c = R.Case(E, D, B, raw=raw)
                inp = R.make_inputs(c)
                lo, hi = R.run_reference(c, inp, torch.float32), R.run_reference(c, inp)
                p = R.Parts(c.name, worst)
                R.check_forward(p, c, lo["joint"], lo["kl"], lo["z"], hi, tol=2e-6)
                R.check_backward(p, c, lo["dheads"], lo["dtheta"], hi, tol=2e-6)
                p.done()
    print(f"E = {E}: float32 against float64, worst per part: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= 2e-6, worst
    # ... which leaves at least 8 x under every bound the device is held to
    bound = {"joint": R.TOL_JOINT, "z": R.TOL_Z, "kl": R.TOL_KL, "kl (one expert)": R.TOL_KL}
    assert all(8 * v <= bound.get(k, R.TOL_GRAD) for k, v in worst.items()), worst


def test_case_tables_cover_what_the_gpu_suite_claims():
    names = {c.name for c in R.ALL_CASES}
    assert {(c.D, c.raw) for c in R.WIDTH_CASES} == {(D, raw) for D in (1, 8, 63, 64, 65, 256) for raw in (False, True)}
    assert {c.E for c in R.EXPERT_CASES if c.D == 8} == {1, 2, 3, 5, 8} and "E8-D256-B7" in names and "E8-D256-B7-raw" in names
    assert {c.B for c in R.ROW_CASES} == {1, 5, 1100}
    assert all(c.spike and c.raw for c in R.SPIKE_CASES) and {c.D <= 64 for c in R.SPIKE_CASES} == {True, False}
    assert all(c.theta0 for c in R.THETA0_CASES) and not any(c.theta0 for c in R.WIDTH_CASES)
    assert {c.B for c in R.THETA_CASES} == {5, 116, 129, 1100} and all(c.E == 1 for c in R.SINGLE_CASES)
    # the launch geometry: one wave per row up to MAX_WAVES waves in workgroups of four, then rows wave, wave + MAX_WAVES, ...
    # -- 1100 rows give a wave its second and its third row; the workspace is one row per workgroup
    from multimodal_vae_comparison_amd import hipops
    L = hipops.lib()
    assert L.mmvae_tc_fusion_ws_floats(1100, 32) == (R.MAX_WAVES // 4) * 32 and 1100 > 2 * R.MAX_WAVES
    assert L.mmvae_tc_fusion_ws_floats(5, 70) == 2 * 70 and L.mmvae_tc_fusion_ws_floats(1, 1) == 1
    assert L.mmvae_tc_fusion_ws_floats(5, 257) == 0 and L.mmvae_tc_fusion_ws_floats(0, 8) == 0


def test_inputs_hold_the_edges_the_gpu_tests_rely_on():
    spike = R.SPIKE_CASES[0]
    inp = R.make_inputs(spike)
    lv = F.softmax(inp["heads"][0][:, spike.D:], -1) + 1e-6
    assert float(lv[3].max()) == pytest.approx(1.0, abs=1e-5) and float(lv[3].min()) == pytest.approx(1e-6, rel=1e-5)
    assert float(lv[2].min()) > 1e-4
    assert not R.make_inputs(R.THETA0_CASES[0])["theta"].any() and R.make_inputs(R.WIDTH_CASES[2])["theta"].any()
    a, b = R.make_inputs(R.WIDTH_CASES[0]), R.make_inputs(R.WIDTH_CASES[0])
    assert all(torch.equal(x, y) for x, y in zip(a["heads"], b["heads"])) and torch.equal(a["gkl"], b["gkl"])
    # upstream gradients that are absent are zeros in the reference too
    c = R.FAMILY_CASES[0]
    inp = R.make_inputs(c)
    none = R.run_reference(c, inp, use_kl=True, use_z=False, rows=())
    assert not any(bool(g.any()) for g in none["dheads"]) and not bool(none["dtheta"].any())
    only_z = R.run_reference(c, inp, use_kl=False)
    assert not bool(only_z["dtheta"].any()) and any(bool(g.any()) for g in only_z["dheads"])


# ---------------------------------------------------------------------------------------------
# the mixer's host side
# ---------------------------------------------------------------------------------------------
def _trainer(mods=None, model_cfg=None, **kw):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods("mvtcae", CD_MODS if mods is None else mods, 8, batch_size=4, **kw)
    if model_cfg is not None:
        cfg["model_cfg"] = model_cfg
    return MultimodalVAE(cfg, feature_dims=dims, device="cpu")


def test_registry_and_alpha():
    from multimodal_vae_comparison_amd import models
    from multimodal_vae_comparison_amd.models.mmvae_models import MVTCAE, POE
    assert models.mvtcae is MVTCAE and "mvtcae" in models.__all__ and issubclass(MVTCAE, POE)
    model = _trainer().model
    assert isinstance(model, MVTCAE) and model.modelName == "mvtcae" and model.alpha == pytest.approx(5.0 / 6.0)
    assert _trainer(model_cfg={"alpha": 0.25}).model.alpha == 0.25
    assert _trainer(model_cfg={"alpha": 0}).model.alpha == 0.0 and _trainer(model_cfg={"alpha": 1}).model.alpha == 1.0
    assert _trainer(model_cfg={}).model.alpha == pytest.approx(5.0 / 6.0)
    for bad in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            _trainer(model_cfg={"alpha": bad})
    # the loss weights: (M - alpha) / M llik on the reconstructions, beta alpha / M per expert row, beta (1 - alpha) on the prior's
    model = _trainer(model_cfg={"alpha": 0.5}, beta=2.5).model
    W = model._tc_weights()
    assert W[0] == pytest.approx([0.75, 0.75, 0.625, 0.625, 1.25]) and W[1] == pytest.approx([0, 0, 0.25, 0.25, 0.5])
    assert W[2] == [0, 0, 0, 0, 1] and W[3] == pytest.approx([0, 0, 0.5, 0.5, 0])


def test_refusals_name_their_cause():
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch
    with pytest.raises(NotImplementedError, match="private_latents"):
        _trainer(mods=[dict(m, private=4) for m in CD_MODS])
    with pytest.raises(NotImplementedError, match="obj 'iwae'"):
        _trainer(obj="iwae")
    with pytest.raises(NotImplementedError, match="K = 4"):
        _trainer(K=4)
    with pytest.raises(NotImplementedError, match="prior 'laplace'"):
        _trainer(prior="laplace")
    model = _trainer().model
    batch = cdsprites_batch(4, 6, seed=3)
    batch["mod_2"] = dict(batch["mod_2"], data=None)
    with pytest.raises(ValueError, match=r"mod_2.*every modality"):
        model.objective(batch)


@pytest.mark.parametrize("given", ["mod_1", "mod_2"])
def test_forward_with_one_modality_returns_that_expert_as_the_joint(given, monkeypatch):
    """no prior expert in the product: with ONE modality present the joint is that modality's expert itself, mean mu and
    scale exp(lv) + 1e-8 (with the N(0, 1) expert POE adds, the mean would shrink towards 0).  The towers and the fusion
    are stood in for by plain torch: this is about which experts modality_mixing multiplies."""
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _trainer().model.eval()
    B, D = 4, 8
    g = torch.Generator().manual_seed(11)
    heads = {m: (torch.randn(B, D, generator=g), F.softmax(torch.randn(B, D, generator=g), -1) + 1e-6) for m in model.vaes}
    calls = []

    def poe(theta, packed, eps, with_prior, kl_mask, gtheta=None, **kw):
        calls.append((len(packed), int(with_prior)))
        return PR.poe_reference(theta, packed, eps, with_prior, kl_mask)

    monkeypatch.setattr(ops, "poe_reparam_kl", poe)
    for m, vae in model.vaes.items():
        vae.enc.forward = lambda x, m=m: heads[m]
        vae.dec.forward = lambda zd: (zd["latents"], torch.ones_like(zd["latents"]))
    batch = cdsprites_batch(B, 6, seed=3)
    for m in batch:
        if m != given:
            batch[m] = dict(batch[m], data=None)
    model.eps_override = [torch.zeros(B, D)]
    out = model.forward(batch)
    assert calls == [(1, 0)]
    mu, lv = heads[given]
    for m in model.vaes:
        joint = out.mods[m].joint_dist
        assert torch.allclose(joint.loc, mu, rtol=1e-6, atol=0) and torch.allclose(joint.scale, torch.exp(lv) + 1e-8, rtol=1e-6)
        assert torch.allclose(out.mods[m].latent_samples["latents"][0], mu, rtol=1e-6, atol=0)      # (eps = 0)
    assert set(out.mods[given].encoder_dist.loc.shape) == {B, D} and out.mods[given].encoder_dist.loc is mu
    assert not math.isclose(float(mu.abs().max()), 0.0)
