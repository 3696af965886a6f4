"""The float64 restatement of the Jensen-Shannon fusion (tests/js_reference.py) against torch's own operations on the CPU,
so that tests/test_js_fusion_gpu.py does not measure the kernel against a mistake: every KL row against
torch.distributions, the geometric-mean property of the dynamic prior, autograd against finite differences, the
restatement in float32 against float64 (where the GPU suite's tolerances come from), the selection rule -- and the host
side of the mmJSD mixer: registry, `prior_weight`, its refusals.  Nothing here reaches a kernel.

Float32 against float64 on the CPU, worst part over E = 1, 2, 3, 5, 8 x D = 1 .. 256 x B = 1, 5, 130 x raw on / off and the
two `spike` cases, each part on its own float64 maximum (printed with -s): prior 3.6e-7, z 7.8e-8, kl rows 1.0e-6, kl
entries (each on its own value) 1.0e-6, dmu 9.3e-7, dsigma 2.4e-6, du 1.4e-6, dtheta 1.1e-6 -- the GPU bounds (1e-5, 1e-5,
2e-5, 5e-5) sit at least 8 x above.  The `spike` rows (expert 0's scale is 1e-6 in all columns but one), their own KL
entries in float32 against float64: 2.7e-7 (D = 32) and 1.2e-7 (D = 70) with m_j from pairwise differences, 1.9e-7 and
8.9e-7 with m_j = mu_j - f."""
import pytest
import torch
import torch.distributions as dist
import torch.nn.functional as F

import js_reference as R

F64 = torch.float64


def _inputs(E, D, B, raw=False, weights="uniform", sel="chunks"):
    inp = R.make_inputs(R.Case(E, D, B, raw=raw), weights, sel)
    return [h.double() for h in inp["heads"]], inp["eps"].double(), inp["theta"].double(), inp["sel"], inp["weights"]


def _experts(heads, theta, D, raw):
    """[(mu_j, sigma_j)] of the E experts and, last, the prior"""
    out = [(h[:, :D], (F.softmax(h[:, D:], -1) + 1e-6) if raw else h[:, D:]) for h in heads]
    return out + [(torch.zeros(1, D, dtype=F64), F.softmax(theta, -1) * D)]


@pytest.mark.parametrize("E,D,raw,weights", [(1, 1, False, "uniform"), (2, 9, False, "half"), (3, 70, True, "unequal"),
                                             (5, 8, False, "uniform"), (8, 16, True, "unequal")])
def test_kl_rows_are_torch_distributions_kl(E, D, raw, weights):
    heads, eps, theta, sel, w = _inputs(E, D, 6, raw, weights)
    prior, kl, z = R.js_reference(theta, heads, eps, sel, w, raw)
    for pairwise in (True, False):
        assert torch.allclose(R.js_reference(theta, heads, eps, sel, w, raw, pairwise)[1], kl, rtol=1e-12, atol=0)
    q = dist.Normal(prior[0], prior[1])
    for j, (mu, sg) in enumerate(_experts(heads, theta, D, raw)):
        want = dist.kl_divergence(dist.Normal(mu.expand(6, D), sg.expand(6, D)), q).sum(-1)
        assert float((kl[j] - want).abs().max()) <= 1e-9, j
    # z: every row from its own expert, MOE's reading of the head (mu + lv eps)
    ex = _experts(heads, theta, D, raw)
    for b in range(6):
        mu, sg = ex[int(sel[b])]
        assert torch.equal(z[b], mu[b] + sg[b] * eps[b])


@pytest.mark.parametrize("E,D,raw,weights", [(1, 3, False, "uniform"), (3, 9, True, "unequal"), (5, 8, False, "half")])
def test_dynamic_prior_is_the_weighted_geometric_mean(E, D, raw, weights):
    """sum_j pi_j log q_j(x) - log N(x; f, P^-1/2) does not depend on x: the same constant, per element, at random points
    (pi sums to 1, so the geometric mean of Gaussians is a Gaussian up to its normaliser)"""
    heads, eps, theta, sel, w = _inputs(E, D, 4, raw, weights)
    prior, _, _ = R.js_reference(theta, heads, eps, sel, w, raw)
    assert sum(w) == pytest.approx(1.0, abs=1e-12)
    g = torch.Generator().manual_seed(3)
    ex = _experts(heads, theta, D, raw)
    consts = []
    for _ in range(5):
        x = torch.randn(4, D, generator=g, dtype=F64) * 2
        mix = sum(pi * dist.Normal(mu, sg).log_prob(x) for pi, (mu, sg) in zip(w, ex))
        consts.append(mix - dist.Normal(prior[0], prior[1]).log_prob(x))
    for c in consts[1:]:
        assert float((c - consts[0]).abs().max()) <= 1e-9


@pytest.mark.parametrize("E,raw,sel", [(1, False, "chunks"), (2, True, "shuffled"), (3, False, "one")])
def test_autograd_matches_finite_differences(E, raw, sel):
    B, D = 3, 3
    g = torch.Generator().manual_seed(5)
    heads = []
    for _ in range(E):
        mu, u = torch.randn(B, D, generator=g, dtype=F64), torch.randn(B, D, generator=g, dtype=F64)
        heads.append(torch.cat([mu, u if raw else F.softmax(u, -1) + 1e-6], -1).requires_grad_(True))
    eps = torch.randn(B, D, generator=g, dtype=F64)
    theta = (torch.randn(1, D, generator=g, dtype=F64) * 0.3).requires_grad_(True)
    s = R.make_selection(R.Case(E, D, B), sel)
    w = R.make_weights(E, "unequal")

    def f(theta, *heads):
        _, kl, z = R.js_reference(theta, list(heads), eps, s, w, raw)
        return kl, z
    assert torch.autograd.gradcheck(f, (theta, *heads), eps=1e-7, atol=1e-6, rtol=1e-5)


def _f32_against_f64(c, worst, weights="uniform", sel="chunks"):
    inp = R.make_inputs(c, weights, sel)
    lo, hi = R.run_reference(c, inp, torch.float32), R.run_reference(c, inp)
    p = R.Parts(c.name, worst)
    R.check_forward(p, c, lo["prior"], lo["kl"], lo["z"], hi, tol=2.5e-6)
    R.check_backward(p, c, lo["dheads"], lo["dtheta"], hi, tol=2.5e-6)
    p.done()


@pytest.mark.parametrize("E", R.EXPERTS)
def test_reference_in_float32_is_within_2_5e_6_of_float64(E):
    """where the tolerances of the GPU suite come from: the restatement evaluated in float32 on the CPU against float64,
    part by part, each on its own float64 maximum (and every KL entry on its own value), over D = 1 .. 256, B = 1 .. 130,
    raw on and off, the three weightings and selections in turn, and the `spike` cases"""
    worst = {}
    k = 0
    for D in R.WIDTHS:
        for B in (1, 5, 130):
            for raw in (False, True):
                if D == 1 and B < 130:
                    # (one element per KL row: every scale is 1 + 1e-6, the row is P m_j^2 / 2 alone and as near 0 as m_j
                    # happens to be -- with one or five rows there is no maximum to measure on; the GPU suite's D = 1
                    # cases have 37 rows)
                    continue
                _f32_against_f64(R.Case(E, D, B, raw=raw), worst, R.WEIGHTS[k % 3], R.SELECTIONS[(k // 3) % 3])
                k += 1
    if E == 2:
        for c in R.SPIKE_CASES:
            _f32_against_f64(c, worst)
    print(f"E = {E}: float32 against float64, worst per part: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    entry = worst.pop("kl entry", 0.0)      # (every KL entry on its own value: held to TOL_KL itself by check_forward)
    assert max(worst.values()) <= 2.5e-6 and entry <= R.TOL_KL, (worst, entry)
    # ... which leaves at least 8 x under every bound the device's parts are held to
    bound = {"prior": R.TOL_JOINT, "z": R.TOL_Z, "kl": R.TOL_KL}
    assert all(8 * v <= bound.get(k, R.TOL_GRAD) for k, v in worst.items()), worst


def test_pairwise_differences_keep_the_saturated_row():
    """the `spike` row: expert 0's scale is 1e-6 in every column but one, P reaches 1e12 and mu_j - f cancels to float32
    rounding before P multiplies its square -- how far off depends on how the division that gives f happens to round.  The
    pairwise form does not depend on that: in float32 that row's own KL entries stay 8 x inside the GPU suite's entry bound.
    (The subtracted form is printed beside it; with torch's float32 division on the CPU it is no worse on these two rows.)"""
    for c in R.SPIKE_CASES:
        inp = R.make_inputs(c)
        hi = R.run_reference(c, inp)["kl"][:, 3]
        err = {}
        for pairwise in (True, False):
            lo = R.run_reference(c, inp, torch.float32, pairwise=pairwise)["kl"][:, 3].double()
            err[pairwise] = float(((lo - hi).abs() / hi.abs()).max())
        print(f"{c.name}, row 3, float32 against float64 on the entries' own values: pairwise {err[True]:.2e}, "
              f"subtracted {err[False]:.2e}")
        assert err[True] <= R.TOL_KL / 8, err


def test_selection_rule():
    """sel[b] = (b M) // B: contiguous chunks whose sizes differ by at most one; B < M leaves experts without a row"""
    from multimodal_vae_comparison_amd.models.mmvae_models import MMJSD
    assert R.chunks(6, 3).tolist() == [0, 0, 1, 1, 2, 2]                  # B % M == 0
    assert R.chunks(3, 3).tolist() == [0, 1, 2]                           # B == M
    assert R.chunks(2, 3).tolist() == [0, 1] and R.chunks(1, 3).tolist() == [0]      # B < M
    assert R.chunks(7, 3).tolist() == [0, 0, 0, 1, 1, 2, 2]               # B % M != 0
    assert R.chunks(5, 2).tolist() == [0, 0, 0, 1, 1]
    for B, M in ((128, 3), (1000, 7), (37, 8)):
        s = R.chunks(B, M)
        counts = torch.bincount(s.long(), minlength=M)
        assert bool((s[1:] >= s[:-1]).all()) and int(counts.max() - counts.min()) <= 1 and s.dtype == torch.int32
    # the mixer builds the same tensor, once per (B, M, device)
    model = _trainer().model
    assert isinstance(model, MMJSD)
    for B in (1, 2, 5, 8):
        s = model._selection(B, torch.device("cpu"))
        assert torch.equal(s, R.chunks(B, 2)) and s.dtype == torch.int32 and model._selection(B, torch.device("cpu")) is s


def test_inputs_and_case_tables():
    names = {c.name for c in R.ALL_CASES}
    assert {(c.D, c.raw) for c in R.WIDTH_CASES} == {(D, raw) for D in (1, 8, 63, 64, 65, 256) for raw in (False, True)}
    assert {c.E for c in R.EXPERT_CASES if c.D == 8} == {1, 2, 3, 5, 8} and "E8-D256-B7" in names and "E8-D256-B7-raw" in names
    assert {c.B for c in R.ROW_CASES} == {1, 5, 1100} and R.B0 == 37
    assert all(c.spike and c.raw for c in R.SPIKE_CASES) and all(c.theta0 for c in R.THETA0_CASES)
    for E in R.EXPERTS:
        for kind in R.WEIGHTS:
            w = R.make_weights(E, kind)
            assert len(w) == E + 1 and min(w) > 0 and sum(w) == pytest.approx(1.0, abs=1e-12)
        assert R.make_weights(E, "half")[E] == 0.5
    w = R.make_weights(3, "unequal")
    assert w[0] < w[1] < w[2]
    c = R.Case(3, 8, R.B0)
    for kind in R.SELECTIONS:
        s = R.make_selection(c, kind)
        assert s.dtype == torch.int32 and s.shape == (c.B,) and 0 <= int(s.min()) and int(s.max()) < c.E
    assert set(R.make_selection(c, "shuffled").tolist()) == {0, 1, 2} and set(R.make_selection(c, "one").tolist()) == {2}
    a, b = R.make_inputs(c, "unequal", "shuffled"), R.make_inputs(c, "unequal", "shuffled")
    assert torch.equal(a["sel"], b["sel"]) and a["weights"] == b["weights"] and torch.equal(a["heads"][0], b["heads"][0])
    # the launch geometry is the tc fusion's: one partial prior-gradient row per workgroup of four waves
    from multimodal_vae_comparison_amd import hipops
    L = hipops.lib()
    assert L.mmvae_js_fusion_ws_floats(1100, 32) == (R.MAX_WAVES // 4) * 32 and 1100 > 2 * R.MAX_WAVES
    assert L.mmvae_js_fusion_ws_floats(5, 70) == 2 * 70 and L.mmvae_js_fusion_ws_floats(1, 1) == 1
    assert L.mmvae_js_fusion_ws_floats(5, 257) == 0 and L.mmvae_js_fusion_ws_floats(0, 8) == 0


def test_an_index_no_expert_has_gives_a_zero_row_in_the_reference():
    c = R.Case(2, 8, 5)
    inp = R.make_inputs(c)
    inp["sel"] = torch.tensor([0, 2, 1, -1, 9], dtype=torch.int32)
    ref = R.run_reference(c, inp, use_kl=False)
    assert not bool(ref["z"][[1, 3, 4]].any()) and bool(ref["z"][[0, 2]].all())
    for e in range(2):
        assert not bool(ref["dheads"][e][[1, 3, 4]].any())
    assert bool(ref["dheads"][0][0].any()) and not bool(ref["dheads"][0][2].any()) and bool(ref["dheads"][1][2].any())


def test_wrapper_checks_sel_and_weights_on_the_host():
    """ops.js_fusion refuses a host-side `sel` outside [0, E) and a weight vector of the wrong length before any kernel"""
    from multimodal_vae_comparison_amd import ops
    heads = [torch.zeros(3, 8) for _ in range(2)]
    theta, eps = torch.zeros(1, 4), torch.zeros(3, 4)
    for bad in ([0, 1, 2], torch.tensor([0, -1, 1]), [0.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="sel"):
            ops.js_fusion(theta, heads, eps, bad, [0.3, 0.3, 0.4])
    with pytest.raises(ValueError, match="weights"):
        ops.js_fusion(theta, heads, eps, [0, 1, 1], [0.5, 0.5])


def test_jsfusion_is_in_the_makefile():
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "Makefile")).read()
    srcs = next(line for line in src.splitlines() if line.startswith("SRCS"))
    assert "jsfusion.hip" in srcs.split()
    assert os.path.exists(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "jsfusion.hip"))


# ---------------------------------------------------------------------------------------------
# the mixer's host side
# ---------------------------------------------------------------------------------------------
def _trainer(mods=None, model_cfg=None, **kw):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods("mmjsd", CD_MODS if mods is None else mods, 8, batch_size=4, **kw)
    if model_cfg is not None:
        cfg["model_cfg"] = model_cfg
    return MultimodalVAE(cfg, feature_dims=dims, device="cpu")


def test_registry_and_prior_weight():
    from multimodal_vae_comparison_amd import models
    from multimodal_vae_comparison_amd.models.mmvae_models import MMJSD, MOE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, step_flops_per_sample
    assert models.mmjsd is MMJSD and "mmjsd" in models.__all__ and issubclass(MMJSD, MOE)
    model = _trainer().model
    assert isinstance(model, MMJSD) and model.modelName == "mmjsd" and model.prior_weight == pytest.approx(1.0 / 3.0)
    assert model._js_pi() == pytest.approx([1.0 / 3.0] * 3)
    assert _trainer(model_cfg={}).model.prior_weight == pytest.approx(1.0 / 3.0)
    assert _trainer(model_cfg={"prior_weight": 0.2}).model._js_pi() == pytest.approx([0.4, 0.4, 0.2])
    for bad in (0, 1, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="prior_weight"):
            _trainer(model_cfg={"prior_weight": bad})
    # the loss weights: llik on the reconstructions, beta pi_e per expert row, beta pi_M on the prior's
    model = _trainer(model_cfg={"prior_weight": 0.5}, beta=2.5).model
    W = model._js_weights()
    assert W[0] == pytest.approx([1.0, 1.0, 0.625, 0.625, 1.25]) and W[1] == pytest.approx([0, 0, 0.25, 0.25, 0.5])
    assert W[2] == [0, 0, 0, 0, 1] and W[3] == pytest.approx([0, 0, 0.5, 0.5, 0])
    # inference and the evaluation hooks are MOE's own
    for name in ("forward", "_sample", "_proposal", "_unimodal", "_proposal_size", "modality_mixing"):
        assert getattr(MMJSD, name) is getattr(MOE, name), name
    # one encoder and one decoder pass per modality in the FLOP count (moe: M decoder passes)
    meta = {"mixing": "mmjsd", "mods": CD_MODS, "D": 16, "T": 32}
    assert step_flops_per_sample(meta) == step_flops_per_sample(dict(meta, mixing="mvtcae"))
    assert step_flops_per_sample(meta) < step_flops_per_sample(dict(meta, mixing="moe"))


def test_refusals_name_their_cause():
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch
    with pytest.raises(NotImplementedError, match="private_latents"):
        _trainer(mods=[dict(m, private=4) for m in CD_MODS])
    with pytest.raises(NotImplementedError, match="obj 'iwae'"):
        _trainer(obj="iwae")
    with pytest.raises(NotImplementedError, match="obj 'dreg'"):
        _trainer(obj="dreg")
    with pytest.raises(NotImplementedError, match="K = 4"):
        _trainer(K=4)
    with pytest.raises(NotImplementedError, match="prior 'laplace'"):
        _trainer(prior="laplace")
    model = _trainer().model
    batch = cdsprites_batch(4, 6, seed=3)
    batch["mod_2"] = dict(batch["mod_2"], data=None)
    with pytest.raises(ValueError, match=r"mod_2.*every modality"):
        model.objective(batch)
