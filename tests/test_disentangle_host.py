"""Host-side tests of the latent disentanglement metrics: properties of the extended-precision
restatement itself (tests/disentangle_reference.py), the two scalar ops on host tensors against it, every refusal of the
three ops and of TorchMMVAE.disentanglement before anything is launched, and the walk of the method on scripted posteriors
in every mixer's own format: which keys appear, in which order, whose noise is used, how the labels lie, and that the noise
setup comes back as it was found.  The models live on the CPU: nothing here reaches a kernel."""
import math

import numpy as np
import pytest
import torch

import disentangle_reference as R

LD = np.longdouble


def _model(mixing="mopoe", mods=None, D=8, prior="normal"):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4, prior=prior)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


@pytest.fixture
def no_launch(monkeypatch):
    """any use of the library fails the test"""
    from multimodal_vae_comparison_amd import hipops

    def lib():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hipops, "lib", lib)


# ---- 1. the restatement itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2])
def test_kl_is_the_sum_of_its_three_parts(i):
    e = R.case(i)["elbo"]
    assert abs(float(e["kl"] - (e["mi"] + e["tc"] + e["dwkl"]))) <= 1e-12
    assert float(e["mi"]) > 0.0 and float(e["mi"]) <= np.log(R.CASES[i][0]) + 1e-12


def test_identical_posteriors_carry_no_information():
    z, loc, scale, labels = R.generate(40, 3, 2, 3, True)
    loc, scale = np.repeat(loc[:1], 40, 0), np.repeat(scale[:1], 40, 0)
    agg = R.aggregate(z, loc, scale, True, labels)
    assert abs(float(R.decomposition(agg, R.log_prior(z))["mi"])) <= 1e-15
    assert float(np.abs(agg["conditional"] - agg["marginal"][None]).max()) <= 1e-15
    assert float(np.abs(R.gap(agg, labels)["mi"]).max()) <= 1e-15


def test_a_factor_with_a_value_per_sample_gives_the_own_term():
    z, loc, scale, _ = R.generate(12, 4, 0, 0, False)
    labels = np.arange(12, dtype=np.int32)[None, ::-1].copy()
    agg = R.aggregate(z, loc, scale, False, labels)
    own = R.pair_terms(z, loc, scale, False)[np.arange(12), np.arange(12)]
    assert bool((agg["counts"] == 1).all()) and float(np.abs(agg["conditional"][0] - own).max()) <= 1e-17
    assert float(np.abs(agg["self"] - own.sum(1)).max()) <= 1e-17


def test_three_points_by_hand():
    """Normal, unit scales, every draw on its own mean: loc = z = (0, 1, 3); classes (0, 0, 1)"""
    z = loc = np.array([[0.0], [1.0], [3.0]], np.float32)
    scale, labels = np.ones((3, 1), np.float32), np.array([[0, 0, 1]], np.int32)
    c, e = 0.5 * math.log(2.0 * math.pi), math.exp
    sums = [1.0 + e(-0.5) + e(-4.5), 1.0 + e(-0.5) + e(-2.0), 1.0 + e(-4.5) + e(-2.0)]
    marginal = np.array([math.log(s) - c - math.log(3.0) for s in sums])
    cond = np.array([math.log(1.0 + e(-0.5)) - c - math.log(2.0)] * 2 + [-c])
    agg = R.aggregate(z, loc, scale, False, labels)
    assert np.abs(np.asarray(agg["marginal"][:, 0], float) - marginal).max() <= 1e-15
    assert np.abs(np.asarray(agg["joint"], float) - marginal).max() <= 1e-15           # (D = 1)
    assert np.abs(np.asarray(agg["conditional"][0, :, 0], float) - cond).max() <= 1e-15
    assert np.abs(np.asarray(agg["self"], float) + c).max() <= 1e-15
    got = R.decomposition(agg, R.log_prior(z))
    assert abs(float(got["mi"]) - (-c - marginal.mean())) <= 1e-15 and abs(float(got["tc"])) <= 1e-18
    h_v = -(2 / 3 * math.log(2 / 3) + 1 / 3 * math.log(1 / 3))
    two = R.aggregate(np.repeat(z, 2, 1), np.repeat(loc, 2, 1), np.repeat(scale, 2, 1) * np.float32([1, 2]), False, labels)
    g = R.gap(two, labels)
    assert abs(float(g["h_v"][0]) - h_v) <= 1e-15
    assert abs(float(g["mi"][0, 0]) - (cond.mean() - marginal.mean())) <= 1e-15
    assert abs(float(g["per_factor"][0]) - float(g["mi"][0, 0] - g["mi"][0, 1]) / h_v) <= 1e-15 and float(g["mig"]) > 0.0


# ---- 2. the scalar ops on host tensors --------------------------------------------------------------------------------------
def _host_agg(c):
    return {k: None if c["agg"][k] is None else torch.from_numpy(np.asarray(c["agg"][k], np.float64))
            for k in ("joint", "marginal", "conditional", "self")}


@pytest.mark.parametrize("i", [1, 2])
def test_scalar_ops_against_the_restatement(no_launch, i):
    from multimodal_vae_comparison_amd import ops
    c = R.case(i)
    N, D = c["z"].shape
    agg, labels = _host_agg(c), torch.from_numpy(np.array(c["labels"]))
    tol = 64 * N * R.U * float(np.abs(np.asarray(c["agg"]["self"], float)).max())      # (float64 inputs, float64 means)
    out = ops.elbo_decomposition(agg, torch.from_numpy(np.asarray(c["lpz"], np.float64)))
    for n in ("mi", "tc", "dwkl", "kl"):
        assert out[n].dtype == torch.float64 and out[n].dim() == 0
        assert abs(float(out[n]) - float(c["elbo"][n])) <= tol
    gap = ops.mutual_information_gap(agg, labels)
    for n in ("per_factor", "mi", "h_z", "h_v"):
        assert np.abs(gap[n].numpy() - np.asarray(c["gap"][n], float)).max() <= tol, n
    assert abs(float(gap["mig"]) - float(c["gap"]["mig"])) <= tol


# ---- 3. the refusals of the ops -----------------------------------------------------------------------------------------------
def test_aggregate_posterior_refuses_before_a_launch(no_launch):
    from multimodal_vae_comparison_amd import ops
    ok, lab = torch.ones(4, 3), torch.zeros(2, 4, dtype=torch.int64)
    nan = ok.clone()
    nan[1, 1] = float("nan")
    for args, kwargs, said in (
            (([[1.0]], ok, ok), {}, "z is list"),
            ((torch.ones(4), ok, ok), {}, r"z is \(4,\)"),
            ((torch.ones(4, 3, dtype=torch.int32), ok, ok), {}, "z is .*int32"),
            ((torch.ones(16385, 1),) * 3, {}, "z is 16385 x 1"),
            ((torch.ones(2, 257),) * 3, {}, "z is 2 x 257"),
            ((torch.ones(0, 3),) * 3, {}, "z is 0 x 3"),
            ((ok, torch.ones(4, 2), ok), {}, "loc is"),
            ((ok, ok, torch.ones(5, 3)), {}, "scale is"),
            ((torch.ones(3, 4).t(), ok, ok), {}, "z is not contiguous"),
            ((ok, nan, ok), {}, "loc holds values that are not finite"),
            ((ok, ok, nan), {}, "scale holds values that are not finite"),
            ((ok, ok, torch.zeros(4, 3)), {}, "scale holds values that are not positive"),
            ((ok, ok, ok), {"labels": torch.zeros(2, 4)}, "labels is .*float32"),
            ((ok, ok, ok), {"labels": torch.zeros(4, dtype=torch.int64)}, "labels is"),
            ((ok, ok, ok), {"labels": torch.zeros(2, 5, dtype=torch.int64)}, r"labels is \(2, 5\)"),
            ((ok, ok, ok), {"labels": torch.zeros(9, 4, dtype=torch.int64)}, r"labels is \(9, 4\)"),
            ((ok, ok, ok), {"labels": torch.zeros(4, 2, dtype=torch.int64).t()}, "labels is not contiguous"),
            ((ok, ok, ok), {"labels": lab - 1}, "labels holds values outside"),
            ((ok, ok, ok), {"chunks": -1}, "chunks = -1"),
            ((ok, ok, ok), {"labels": lab}, "z is on cpu")):
        with pytest.raises(ValueError, match=f"aggregate_posterior: {said}"):
            ops.aggregate_posterior(*args, **kwargs)


def test_scalar_ops_refuse(no_launch):
    from multimodal_vae_comparison_amd import ops
    agg = _host_agg(R.case(1))
    labels = torch.from_numpy(np.array(R.case(1)["labels"]))
    lpz = torch.zeros(70, dtype=torch.float64)
    for bad_agg, bad_lpz, said in (([], lpz, "agg must be the dict"), ({"joint": agg["joint"]}, lpz, "agg must be the dict"),
                                   (dict(agg, joint=agg["joint"].float()), lpz, r"agg\['joint'\]"),
                                   (dict(agg, self=agg["self"][:5]), lpz, "agg holds"),
                                   (dict(agg, conditional=agg["conditional"][:, :5]), lpz, r"agg\['conditional'\]"),
                                   (agg, lpz[:5], "lpz is"), (agg, [0.0] * 70, "lpz is list"),
                                   (agg, torch.full((70,), float("nan")), "lpz holds")):
        with pytest.raises(ValueError, match=f"elbo_decomposition: {said}"):
            ops.elbo_decomposition(bad_agg, bad_lpz)
    one = {"joint": agg["joint"], "marginal": agg["marginal"][:, :1].contiguous(), "self": agg["self"],
           "conditional": agg["conditional"][:, :, :1].contiguous()}
    for bad_agg, bad_labels, said in ((dict(agg, conditional=None), labels, "agg holds no conditional"), (one, labels, "D = 1"),
                                      (agg, labels[:1], "labels has 1 factors"), (agg, labels.float(), "labels is"),
                                      (agg, labels[:, :5].contiguous(), "labels is"), (agg, labels * 0, "factor 0 .* single value"),
                                      (agg, labels - 5, "labels holds values outside")):
        with pytest.raises(ValueError, match=f"mutual_information_gap: {said}"):
            ops.mutual_information_gap(bad_agg, bad_labels)


# ---- 4. the method: refusals ---------------------------------------------------------------------------------------------------
def test_unimodal_vae_refuses_disentanglement_by_name():
    from multimodal_vae_comparison_amd.models.vae import VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE)
    with pytest.raises(NotImplementedError) as e:
        vae.disentanglement()
    assert "unimodal" in str(e.value) and "TorchMMVAE.disentanglement" in str(e.value)


def test_disentanglement_refuses_before_the_first_forward(no_launch, monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import MS_MODS, cdsprites_batch, mnist_svhn_batch
    model = _model()

    def sample(*a, **k):
        raise AssertionError("a forward ran")
    monkeypatch.setattr(model, "_sample", sample)
    batches = [cdsprites_batch(4, 6, seed=3), cdsprites_batch(2, 6, seed=4)]
    lacking = dict(batches[1], mod_2=dict(batches[1]["mod_2"], data=None))
    huge = {m: dict(v, data=torch.zeros(16385, 1)) for m, v in batches[0].items()}
    good = torch.arange(6).reshape(6, 1) % 2
    mine = model.eps_override = [torch.zeros(4, 8)]
    for args, kwargs, said in (
            (([],), {}, "`batches` is empty"),
            (([batches[0], lacking],), {}, "every batch must hold every modality"),
            (([batches[0], {"mod_1": batches[1]["mod_1"]}],), {}, "every batch must hold every modality"),
            (([huge],), {}, "16385 rows"),
            ((batches,), {"chunks": -2}, "chunks = -2"),
            ((batches,), {"labels": torch.zeros(5, 1, dtype=torch.int64)}, r"labels is \(5, 1\), the batches hold 6 rows"),
            ((batches,), {"labels": good.t()}, r"labels is \(1, 6\), the batches hold 6 rows"),
            ((batches,), {"labels": torch.zeros(6, 9, dtype=torch.int64)}, r"labels is \(6, 9\)"),
            ((batches,), {"labels": good.float()}, "labels must be an integer"),
            ((batches,), {"labels": good - 1}, "labels holds negative values"),
            ((batches,), {"labels": good * 0}, "factor 0 of labels takes a single value"),
            ((batches,), {"eps": {"mod_3": torch.zeros(6, 8)}}, "eps maps"),
            ((batches,), {"eps": {"mod_1": torch.zeros(4, 8)}}, "eps maps")):
        with pytest.raises(ValueError, match=f"disentanglement: {said}"):
            model.disentanglement(*args, **kwargs)
        assert model.eps_override is mine and len(mine) == 1 and model._eval_draws is False
    model.train()
    with pytest.raises(RuntimeError, match="disentanglement needs eval mode"):
        model.disentanglement(batches)
    narrow = _model(mods=MS_MODS, D=1)
    monkeypatch.setattr(narrow, "_sample", sample)
    with pytest.raises(ValueError, match="disentanglement: the mutual information gap needs D >= 2"):
        narrow.disentanglement([mnist_svhn_batch(6, seed=3)], labels=good)


# ---- 5. the method: the walk on scripted posteriors ----------------------------------------------------------------------------
def _script(model, mixing, monkeypatch, fail=False):
    """`_sample` replaced by a script that hands out seeded posteriors in the mixer's own format (the real `_unimodal` and
    `_joint_posterior` read them); the device ops replaced by host stand-ins that record what they are handed
    -> (what was recorded, {key: [(loc, scale) per batch]})"""
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.models.mmvae_base import normal
    names, D = list(model.vaes.keys()), model.n_latents
    g = torch.Generator().manual_seed(5)
    seen = {"read": 0, "inside": [], "agg": [], "draws": []}
    posts = {k: [] for k in names + ["joint"]}

    def sample(x, K=1, of=None):
        assert model._eval_draws is True and model.eps_override is None and not torch.is_grad_enabled()
        B = len(x[names[0]]["data"])
        post = {k: (torch.randn(B, D, generator=g), torch.rand(B, D, generator=g) + 0.3) for k in names + ["joint"]}
        for k, v in post.items():
            posts[k].append(v)
        joint = post["joint"]
        if mixing == "mopoe":
            head = {"modalities": {m: {"shared": post[m]} for m in names}, "joint": list(joint)}
        elif mixing == "poe":
            head = (normal(*joint), {m: normal(*post[m]) for m in names})
        elif mixing == "moe":
            head = {m: normal(*post[m]) for m in names}
        else:
            head = ({m: {"shared": list(post[m]), "private": None} for m in names}, joint, torch.zeros(1, B, D))

        def drawn():
            for m in names:
                yield m, torch.zeros(1, B, D)
            seen["read"] += 1
        return head, drawn()

    def aggregate_posterior(z, loc, scale, laplace=False, labels=None, chunks=0):
        if fail:
            raise RuntimeError("scripted failure")
        seen["agg"].append({"z": z, "loc": loc, "scale": scale, "laplace": laplace, "labels": labels, "chunks": chunks})
        agg = R.aggregate(z.numpy(), loc.numpy(), scale.numpy(), laplace, None if labels is None else labels.numpy())
        return {k: None if agg[k] is None else torch.from_numpy(np.asarray(agg[k], np.float64))
                for k in ("joint", "marginal", "conditional", "self")}

    def draw(family):
        def f(shape, state):
            seen["draws"].append((family, tuple(shape), state))
            return torch.full(shape, 0.5)
        return f
    monkeypatch.setattr(model, "_sample", sample)
    monkeypatch.setattr(ops, "aggregate_posterior", aggregate_posterior)
    monkeypatch.setattr(ops, "randn", draw("normal"))
    monkeypatch.setattr(ops, "rand_laplace", draw("laplace"))
    return seen, posts


def _batches():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    return [cdsprites_batch(4, 6, seed=3), cdsprites_batch(3, 6, seed=4)]


@pytest.mark.parametrize("mixing,prior", [("mopoe", "normal"), ("poe", "normal"), ("moe", "normal"), ("moe", "laplace"),
                                          ("dmvae", "normal")])
def test_walk_keys_noise_and_labels(no_launch, monkeypatch, mixing, prior):
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    mods = [dict(m, private=4) for m in CD_MODS] if mixing == "dmvae" else None
    model = _model(mixing, mods=mods, prior=prior)
    seen, posts = _script(model, mixing, monkeypatch)
    names, N, D = list(model.vaes.keys()), 7, 8
    keys = names + (["joint"] if mixing in ("poe", "dmvae") else [])
    labels = torch.stack([torch.arange(N) % 2, torch.arange(N) % 3, (torch.arange(N) > 2).long()], 1)      # (N, K = 3)
    given = {names[1]: torch.randn(N, D, generator=torch.Generator().manual_seed(9))}
    mine = model.eps_override = [torch.zeros(4, D)]

    out = model.disentanglement(_batches(), labels=labels, eps=given, chunks=3)
    assert model.eps_override is mine and len(mine) == 1 and model._eval_draws is False and torch.is_grad_enabled()
    assert list(out) == keys and seen["read"] == 2 and len(seen["agg"]) == len(keys)
    lap = mixing == "moe" and prior == "laplace"
    for key, handed in zip(keys, seen["agg"]):
        r = out[key]
        loc, scale = (torch.cat([p[i] for p in posts[key]]) for i in (0, 1))
        assert torch.equal(r["loc"], loc) and torch.equal(r["scale"], scale) and r["z"] is handed["z"]
        e = given[key] if key in given else torch.full((N, D), 0.5)
        assert torch.equal(r["z"], loc + scale * e)
        assert handed["laplace"] is (lap and key != "joint") and handed["chunks"] == 3
        assert handed["labels"].shape == (3, N) and torch.equal(handed["labels"], labels.t())       # one ROW per factor
        assert set(r) == {"mi", "tc", "dwkl", "kl", "mig", "per_factor", "mi_table", "h_z", "z", "loc", "scale"}
        assert r["per_factor"].shape == (3,) and r["mi_table"].shape == (3, D) and r["h_z"].shape == (D,)
        assert abs(float(r["kl"] - (r["mi"] + r["tc"] + r["dwkl"]))) <= 1e-12
    # one draw per key without eps, of the key's family, from the evaluation generator
    assert [d[:2] for d in seen["draws"]] == [("laplace" if lap and k != "joint" else "normal", (N, D))
                                              for k in keys if k not in given]
    assert all(d[2] is model._eval_rng_state for d in seen["draws"])
    if mixing not in ("poe", "dmvae"):
        with pytest.raises(ValueError, match="disentanglement: eps\\['joint'\\] given"):
            model.disentanglement(_batches(), eps={"joint": torch.zeros(N, D)})
    plain = model.disentanglement(_batches())
    assert list(plain) == keys and all(set(r) == {"mi", "tc", "dwkl", "kl", "h_z", "z", "loc", "scale"} for r in plain.values())
    assert seen["agg"][-1]["labels"] is None


def test_a_failing_walk_leaves_the_noise_setup_as_it_found_it(no_launch, monkeypatch):
    model = _model("poe")
    _script(model, "poe", monkeypatch, fail=True)
    mine = model.eps_override = [torch.zeros(4, 8)]
    with pytest.raises(RuntimeError, match="scripted failure"):
        model.disentanglement(_batches(), eps={"joint": torch.zeros(7, 8)})
    assert model.eps_override is mine and len(mine) == 1 and model._eval_draws is False and torch.is_grad_enabled()
