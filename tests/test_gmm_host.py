"""Host-side checks of the latent density estimation: the float64 restatement the GPU tests compare
against (tests/gmm_reference.py) is held to scikit-learn's GaussianMixture from the same start, full and diagonal, with an
empty start component; no iteration of any case sits on the knife edge of `tol` (which is what lets the GPU test demand an equal
n_iter); gmm_information against scikit-learn's bic / aic; every argument refusal of the ops and of the two mixin methods on
a CPU model.  Nothing here reaches a kernel."""
import numpy as np
import pytest
import torch

import gmm_reference as R

SK_CASES = [(s, kind) for s in R.SKLEARN_SHAPES for kind in R.KINDS] + [("empty", kind) for kind in R.KINDS]


@pytest.fixture(autouse=True)
def the_ops_under_test_exist():
    """the restatement and its guards are yardsticks for these ops: without them no test here says anything"""
    from multimodal_vae_comparison_amd import ops
    assert all(callable(getattr(ops, name, None)) for name in ("gmm_fit", "gmm_score", "gmm_sample", "gmm_information"))


def _sk_case(shape):
    if shape == "empty":
        X, start, C = R.case(R.EMPTY)
        return np.array(X), np.array(start), C
    N, D, C = shape
    X, start, _ = R.blobs(N, D, C, R.SEED + 200 + N)
    return X, start, C


def _sklearn_from(X, start, C, kind):
    """GaussianMixture pinned to the restatement's start: weights, means and precisions of the one-hot M-step"""
    from sklearn.mixture import GaussianMixture
    X64 = X.astype(np.float64)
    resp = np.zeros((len(X), C))
    resp[np.arange(len(X)), start] = 1.0
    w, means, cov = R.m_step(X64, resp, kind, R.REG)
    _, P, _ = R.factors(cov, kind)
    precisions = np.stack([p @ p.T for p in P]) if kind == "full" else P ** 2
    gm = GaussianMixture(n_components=C, covariance_type=kind, tol=R.TOL, reg_covar=R.REG, max_iter=R.MAX_ITER, n_init=1,
                         weights_init=w, means_init=means, precisions_init=precisions)
    return gm.fit(X64), X64


# ---- a. the restatement against scikit-learn ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", SK_CASES, ids=[f"{s}-{k}" for s, k in SK_CASES])
def test_restatement_against_scikit_learn(shape, kind):
    """n_iter and converged: equal.  Values: within 1e-10 of the quantity's largest magnitude.  The two differ in where they
    round, not in what they compute: scikit-learn rebuilds the start's precision factor from `precisions_init` by a second
    Cholesky factorisation (of the precision, condition number up to 1 / reg_covar = 1e6 for an empty component: 1e6 x 2^-53 =
    1e-10), forms x P - mu P (full) and the expanded square (diag) where the restatement forms (x - mu) P, and sums in
    BLAS's order; the M-step then contracts the difference."""
    X, start, C = _sk_case(shape)
    gm, X64 = _sklearn_from(X, start, C, kind)
    ref = R.em(X, start, C, kind)
    assert not ref["degenerate"]
    figures = {"lower_bound": (ref["lower_bound"], gm.lower_bound_), "weights": (ref["weights"], gm.weights_),
               "means": (ref["means"], gm.means_), "covariances": (ref["covariances"], gm.covariances_),
               "precisions_cholesky": (ref["precisions_cholesky"], gm.precisions_cholesky_),
               "log_density": (ref["log_density"], gm.score_samples(X64)), "resp": (ref["resp"], gm.predict_proba(X64))}
    off = {k: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1.0)) for k, (a, b) in figures.items()}
    print(f"{shape} {kind}: n_iter {ref['n_iter']} / {gm.n_iter_}, converged {ref['converged']} / {gm.converged_}; relative "
          f"differences {({k: f'{v:.2e}' for k, v in off.items()})}; knife edge {R.knife_edge(ref):.3g} of tol")
    assert ref["n_iter"] == gm.n_iter_ and ref["converged"] == gm.converged_
    assert np.array_equal(ref["labels"], gm.predict(X64))
    assert all(v <= 1e-10 for v in off.values()), off
    if shape == "empty":
        assert ref["weights"][2] < 1e-15 and np.array_equal(ref["covariances"][2], np.eye(7) * R.REG if kind == "full" else np.full(7, R.REG))


# ---- b. no case on the knife edge ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("i", range(len(R.SHAPES) + 1), ids=R.case_ids())
def test_no_iteration_on_the_knife_edge_and_no_row_between_two_components(i, kind):
    """what makes equal n_iter, converged and labels a fair demand of the kernels, from the restatement alone"""
    ref = R.fit(i, kind)
    edge = R.knife_edge(ref)
    print(f"{R.case_ids()[i]} {kind}: n_iter {ref['n_iter']}, converged {ref['converged']}, the nearest |change| is {edge:.3g} of "
          f"tol away from tol; smallest gap of a row's two largest responsibilities {ref['gap']:.3g}; spreads "
          f"{({k: f'{v:.2e}' for k, v in ref['spread'].items()})}; tolerances {({k: f'{v:.2e}' for k, v in ref['tol'].items()})}")
    assert edge >= 0.01, "an iteration's change is within 1 % of tol: choose other inputs"
    assert ref["gap"] >= 1e-6, "a row sits between two components: choose other inputs"


@pytest.mark.parametrize("shape,kind", SK_CASES, ids=[f"{s}-{k}" for s, k in SK_CASES])
def test_no_scikit_learn_case_on_the_knife_edge(shape, kind):
    X, start, C = _sk_case(shape)
    assert R.knife_edge(R.em(X, start, C, kind)) >= 0.01


# ---- c. BIC / AIC ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_information_against_scikit_learn(kind):
    from multimodal_vae_comparison_amd import ops
    X, start, C = _sk_case((130, 7, 3))
    gm, X64 = _sklearn_from(X, start, C, kind)
    dens = torch.from_numpy(np.stack([np.zeros(len(X)), gm.score_samples(X64)]))      # (restart 1 holds scikit-learn's rows)
    fit = {"means": torch.zeros(2, C, 7, dtype=torch.float64), "log_density": dens, "covariance_type": kind, "best": 1}
    got = ops.gmm_information(fit, len(X))
    assert got["n_parameters"] == gm._n_parameters() == R.information(C, 7, kind, 0.0, len(X))["n_parameters"]
    assert got["n_parameters"] == (3 * 28 + 21 + 2 if kind == "full" else 42 + 2)
    for name, want in (("bic", gm.bic(X64)), ("aic", gm.aic(X64))):
        assert abs(got[name] - want) <= 4 * np.spacing(abs(want)), (name, got[name], want)
    assert ops.gmm_information(fit, len(X), restart=0)["bic"] == got["n_parameters"] * np.log(len(X))
    single = {"means": fit["means"][1], "score": float(dens[1].numpy().mean()), "covariance_type": kind}
    assert ops.gmm_information(single, len(X)) == got


# ---- d. refusals ---------------------------------------------------------------------------------------------------------------------
def _fit(R_=2, C=3, D=4, N=6, kind="full"):
    shape = (D, D) if kind == "full" else (D,)
    f64 = torch.float64
    return {"weights": torch.full((R_, C), 1.0 / C, dtype=f64), "means": torch.zeros(R_, C, D, dtype=f64),
            "cholesky": torch.ones(R_, C, *shape, dtype=f64), "precisions_cholesky": torch.ones(R_, C, *shape, dtype=f64),
            "log_det": torch.zeros(R_, C, dtype=f64), "log_density": torch.zeros(R_, N, dtype=f64),
            "degenerate": torch.tensor([False, True][:R_]), "best": 0, "covariance_type": kind}


def test_ops_refuse_before_a_launch():
    from multimodal_vae_comparison_amd import ops
    x = torch.ones(6, 4)
    lab = torch.tensor([[0, 1, 2, 0, 1, 2]])
    for match, X in ((r"X is \(6,\)", torch.ones(6)), ("X is .*int64", torch.ones(6, 4, dtype=torch.int64)),
                     ("X has D = 65 dimensions .*MI355X path", torch.ones(6, 65)),
                     ("X has 16385 rows .*MI355X path", torch.ones(16385, 2)),
                     ("X holds values that are not finite", torch.full((6, 4), float("nan")))):
        with pytest.raises(ValueError, match="gmm_fit: " + match):
            ops.gmm_fit(X, lab)
        with pytest.raises(ValueError, match="gmm_score: " + match):
            ops.gmm_score(X, _fit(D=X.shape[1] if X.dim() == 2 and X.shape[1] <= 64 else 4))
    for match, init, kw in (("init is .*float32", lab.float(), {}), (r"init is \(6,\)", lab[0], {}), ("init is list", [[0] * 6], {}),
                            ("init is .*bool", lab > 0, {}), (".*65 restarts .*MI355X path", lab.repeat(65, 1), {}),
                            ("init has 5 labels per restart for 6 rows", lab[:, :5], {}),
                            (".*65 components .*MI355X path", lab + 62, {}),
                            (".*65 components .*MI355X path", lab, {"n_components": 65}),
                            (".*0 components .*MI355X path", lab, {"n_components": 0}),
                            (".*ids -1 .. 1; n_components = 2", lab - 1, {}),
                            (".*ids 0 .. 2; n_components = 2", lab, {"n_components": 2}),
                            ("covariance_type = 'tied'", lab, {"covariance_type": "tied"}),
                            ("reg_covar = -1.0", lab, {"reg_covar": -1.0}), ("reg_covar = nan", lab, {"reg_covar": float("nan")}),
                            ("tol = -0.5", lab, {"tol": -0.5}), ("tol = inf", lab, {"tol": float("inf")}),
                            ("max_iter = 0 .*MI355X path", lab, {"max_iter": 0}),
                            ("max_iter = 1001 .*MI355X path", lab, {"max_iter": 1001}),
                            ("sync_every = 0", lab, {"sync_every": 0}), ("slice_bytes = 0", lab, {"slice_bytes": 0})):
        with pytest.raises(ValueError, match="gmm_fit: " + match):
            ops.gmm_fit(x, init, **kw)
    with pytest.raises(ValueError, match="gmm_fit: X is on cpu.*there is no host path"):
        ops.gmm_fit(x, lab)

    fit = _fit()
    for match, f, kw in (("fit is what gmm_fit returns", [1], {}), ("fit is what gmm_fit returns", dict(fit, means=None), {}),
                         ("fit is what gmm_fit returns", dict(fit, weights=fit["weights"].float()), {}),
                         ("fit is what gmm_fit returns", {k: v for k, v in fit.items() if k != "covariance_type"}, {}),
                         ("covariance_type = 'tied'", dict(fit, covariance_type="tied"), {}),
                         (r"restart = 2 .*restarts 0 \.\. 1", fit, {"restart": 2}), ("restart = -1", fit, {"restart": -1}),
                         ("restart = 0.5", fit, {"restart": 0.5}), ("restart 1 is degenerate", fit, {"restart": 1}),
                         (r"fit holds weights \(3,\), means \(3, 4\), factors \(3, 4, 4\); .*\(C, D\) with", dict(fit, covariance_type="diag"), {}),
                         (r"fit holds weights \(3,\), means \(3, 5\)", dict(fit, means=torch.zeros(2, 3, 5, dtype=torch.float64)), {}),
                         ("restart = 0 for a single mixture", {k: (v[0] if torch.is_tensor(v) else v) for k, v in fit.items()},
                          {"restart": 0})):
        with pytest.raises(ValueError, match="gmm_score: " + match):
            ops.gmm_score(x, f, **kw)
        with pytest.raises(ValueError, match="gmm_sample: " + match):
            ops.gmm_sample(f, 3, u=torch.zeros(3, dtype=torch.float64), eps=torch.zeros(3, 4), **kw)
    with pytest.raises(ValueError, match="gmm_score: X has D = 5 dimensions, the mixture 4"):
        ops.gmm_score(torch.ones(6, 5), fit)
    with pytest.raises(ValueError, match="gmm_score: X is on cpu.*there is no host path"):
        ops.gmm_score(x, fit)

    u, eps = torch.zeros(3, dtype=torch.float64), torch.zeros(3, 4)
    for match, n, kw in (("n = 0 draws", 0, {"u": u, "eps": eps}), (f"n = {2 ** 24 + 1} draws", 2 ** 24 + 1, {"u": u, "eps": eps}),
                         ("u is .*float32", 3, {"u": u.float(), "eps": eps}), (r"u is \(2,\)", 3, {"u": u[:2], "eps": eps}),
                         ("u is list", 3, {"u": [0.0] * 3, "eps": eps}),
                         ("u holds values outside", 3, {"u": torch.tensor([0.0, 1.0, 0.5], dtype=torch.float64), "eps": eps}),
                         ("u holds values outside", 3, {"u": torch.tensor([0.0, -0.1, 0.5], dtype=torch.float64), "eps": eps}),
                         ("u holds values outside", 3, {"u": torch.tensor([0.0, float("nan"), 0.5], dtype=torch.float64), "eps": eps}),
                         ("without eps the draws need `state`", 3, {"u": u}),
                         ("without eps the draws need `state`", 3, {"u": u, "state": torch.zeros(3)}),
                         (r"eps is \(3, 5\)", 3, {"u": u, "eps": torch.zeros(3, 5)}),
                         ("eps is .*int64", 3, {"u": u, "eps": torch.zeros(3, 4, dtype=torch.int64)}),
                         ("eps holds values that are not finite", 3, {"u": u, "eps": torch.full((3, 4), float("inf"))})):
        with pytest.raises(ValueError, match="gmm_sample: " + match):
            ops.gmm_sample(fit, n, **kw)
    with pytest.raises(ValueError, match="gmm_sample: the mixture is on cpu.*there is no host path"):
        ops.gmm_sample(fit, 3, u=u, eps=eps)
    with pytest.raises(ValueError, match="gmm_sample: the mixture is on cpu"):
        ops.gmm_sample(fit, 3, eps=eps)      # (u drawn on the host)

    for match, f, n, kw in (("fit is what gmm_fit returns", [1], 6, {}), ("covariance_type = 'tied'", dict(fit, covariance_type="tied"), 6, {}),
                            ("n_rows = 0", fit, 0, {}), ("restart = 2", fit, 6, {"restart": 2}),
                            ("n_rows = 7, the fit holds the log-density of 6 rows", fit, 7, {}),
                            ("restart = 0 for a single mixture", dict(fit, means=fit["means"][0], score=0.0), 6, {"restart": 0})):
        with pytest.raises(ValueError, match="gmm_information: " + match):
            ops.gmm_information(f, n, **kw)


def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


def test_mixin_argument_errors_come_before_the_first_encoder_call(monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    calls = []
    monkeypatch.setattr(model, "_sample", lambda *a, **kw: calls.append(1))
    monkeypatch.setattr(model, "latents_for", lambda *a, **kw: calls.append(1))
    lacking = dict(batch, mod_2=dict(batch["mod_2"], data=None))
    cases = [
        ("`batches` is empty", ([], 2), {}),
        ("`held_out` is empty", ([batch], 2), {"held_out": []}),
        ("without data", ([lacking], 2), {}),
        ("without data", ([batch], 2), {"held_out": [lacking]}),
        ("must name modalities", ([batch], 2), {"given": [["mod_9"]]}),
        ("must name modalities", ([batch], 2), {"given": [[]]}),
        ("n_components = 0 .*MI355X path", ([batch], 0), {}),
        ("n_components = 65 .*MI355X path", ([batch] * 20, 65), {}),
        ("n_components = 5 for 4 rows", ([batch], 5), {}),
        ("n_init = 0.*MI355X path", ([batch], 2), {"n_init": 0}),
        ("n_init = 65.*MI355X path", ([batch], 2), {"n_init": 65}),
        ("kmeans_iter = 1001.*MI355X path", ([batch], 2), {"kmeans_iter": 1001}),
        ("max_iter = 1001 .*MI355X path", ([batch], 2), {"max_iter": 1001}),
        ("max_iter = 0 .*MI355X path", ([batch], 2), {"max_iter": 0}),
        ("tol = -1.0", ([batch], 2), {"tol": -1.0}),
        ("reg_covar = -1.0", ([batch], 2), {"reg_covar": -1.0}),
        ("covariance_type = 'spherical'", ([batch], 2), {"covariance_type": "spherical"}),
        ("labels must be an integer", ([batch], 2), {"labels": torch.zeros(4)}),
        (r"labels is \(3, 1\), the batches hold 4 rows", ([batch], 2), {"labels": torch.tensor([0, 1, 0])}),
        ("negative values", ([batch], 2), {"labels": torch.tensor([0, 1, -1, 0])}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="fit_latent_density: .*" + match):
            model.fit_latent_density(*args, **kwargs)
    big = dict(batch, mod_1=dict(batch["mod_1"], data=torch.zeros(1, 3, 64, 64).expand(16385, 3, 64, 64)))
    with pytest.raises(ValueError, match="fit_latent_density: 16385 rows .*MI355X path"):
        model.fit_latent_density([big], 2)
    with pytest.raises(ValueError, match="fit_latent_density: `held_out` holds more than 16384 rows"):
        model.fit_latent_density([batch], 2, held_out=[big])
    wide = _model(D=66)      # (the text decoder's two heads want an even width)
    with pytest.raises(ValueError, match="fit_latent_density: 4 rows of 66 latent dimensions .*MI355X path"):
        wide.fit_latent_density([batch], 2)

    f64 = torch.float64
    entry = {"weights": torch.full((3,), 1 / 3, dtype=f64), "means": torch.zeros(3, 8, dtype=f64),
             "cholesky": torch.ones(3, 8, 8, dtype=f64), "precisions_cholesky": torch.ones(3, 8, 8, dtype=f64),
             "log_det": torch.zeros(3, dtype=f64), "covariance_type": "full"}
    for match, d, n, kw in (("n = 0", entry, 0, {}), ("density is one subset's entry", {"mod_1": entry}, 4, {}),
                            ("density is one subset's entry", dict(entry, weights=entry["weights"][None]), 4, {}),
                            ("the density has D = 7 dimensions, the model 8", dict(entry, means=entry["means"][:, :7]), 4, {})):
        with pytest.raises(ValueError, match="sample_latent_density: " + match):
            model.sample_latent_density(d, n, **kw)
    # the ops' own refusals pass through, the last of them the missing device
    with pytest.raises(ValueError, match="gmm_sample: u holds values outside"):
        model.sample_latent_density(entry, 2, u=torch.ones(2, dtype=f64), eps=torch.zeros(2, 8))
    with pytest.raises(ValueError, match="gmm_sample: the mixture is on cpu"):
        model.sample_latent_density(entry, 2, eps=torch.zeros(2, 8))
    assert not calls and model._eval_draws is False and model.eps_override is None


def test_train_mode_and_private_latents_are_refused():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="fit_latent_density needs eval mode"):
        model.fit_latent_density([cdsprites_batch(4, 6, seed=3)], 2)
    with pytest.raises(RuntimeError, match="sample_latent_density needs eval mode"):
        model.sample_latent_density({}, 2)
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    dmvae = _model("dmvae", mods=[dict(m, private=2) for m in CD_MODS])
    assert dmvae.latent_factorization
    with pytest.raises(NotImplementedError, match="sample_latent_density is built for the mixers with one shared latent space"):
        dmvae.sample_latent_density({}, 2)


# ---- e. the unimodal VAE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fit_latent_density", "sample_latent_density"])
def test_unimodal_vae_refuses_both_by_name(name):
    from multimodal_vae_comparison_amd.models.vae import MIXER_METRICS, VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE) and name in MIXER_METRICS
    with pytest.raises(NotImplementedError) as e:
        getattr(vae, name)()
    text = str(e.value)
    assert "unimodal" in text and name in text and f"TorchMMVAE.{name}" in text


# ---- the ABI and the logged names ------------------------------------------------------------------------------------------------------
def test_new_symbols_limits_and_log_tags(monkeypatch):
    import os
    import re
    from conftest import ROOT
    from multimodal_vae_comparison_amd import hipops
    header = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in ("mmvae_gmm_ws_doubles", "mmvae_gmm_em", "mmvae_gmm_score", "mmvae_gmm_sample"):
        assert name in hipops.SIGNATURES and re.search(r"\b" + name + r"\(", header)
    for define, value in (("MMVAE_GMM_MAX_D", hipops.GMM_MAX_D), ("MMVAE_GMM_MAX_DRAWS", hipops.GMM_MAX_DRAWS),
                          ("MMVAE_GMM_FULL", hipops.GMM_COVARIANCES["full"]), ("MMVAE_GMM_DIAG", hipops.GMM_COVARIANCES["diag"])):
        assert int(re.search(r"#define " + define + r" (\d+)", header).group(1)) == value
    L = hipops.lib()
    # record + stamps + n_k + norm sums + moment partials + covariance partials, per restart
    assert L.mmvae_gmm_ws_doubles(130, 7, 3, 2, 0) == 2 * (4 + 64 + 3 + 3 + 3 * 3 * 8 + 3 * 1 * 49)
    assert L.mmvae_gmm_ws_doubles(1100, 7, 3, 1, 1) == 4 + 64 + 3 + 18 + 18 * 3 * 8 + 3 * 2 * 7
    for bad in ((0, 7, 3, 1, 0), (16385, 7, 3, 1, 0), (10, 0, 3, 1, 0), (10, 65, 3, 1, 0), (10, 7, 0, 1, 0), (10, 7, 65, 1, 0),
                (10, 7, 3, 0, 0), (10, 7, 3, 65, 0), (10, 7, 3, 1, 2)):
        assert L.mmvae_gmm_ws_doubles(*bad) == 0

    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods("mopoe", CD_MODS, 8, batch_size=4)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cpu")
    agree = {"ari": 0.5, "nmi": 0.25, "homogeneity": 0.0, "completeness": 0.0, "purity": 0.75}
    fake = {"mod_1": {"score": -1.0, "bic": 10.0, "aic": 8.0, "held_out_score": None, "agreement": {}},
            "mod_1+mod_2": {"score": -2.0, "bic": 20.0, "aic": 16.0, "held_out_score": -3.0, "agreement": {1: agree}}}
    seen = {}
    monkeypatch.setattr(tr.model, "fit_latent_density", lambda batches, C, **kw: seen.update(kw, C=C) or fake)
    assert tr.fit_latent_density(["b"], 3, n_init=2) is fake and seen == {"n_init": 2, "C": 3}
    assert {k: float(v) for k, v in tr.logged.items() if k.startswith("test_density_")} == {
        "test_density_score_mod_1": -1.0, "test_density_bic_mod_1": 10.0, "test_density_aic_mod_1": 8.0,
        "test_density_score_mod_1+mod_2": -2.0, "test_density_bic_mod_1+mod_2": 20.0, "test_density_aic_mod_1+mod_2": 16.0,
        "test_density_held_out_mod_1+mod_2": -3.0, "test_density_ari_mod_1+mod_2_1": 0.5,
        "test_density_nmi_mod_1+mod_2_1": 0.25, "test_density_purity_mod_1+mod_2_1": 0.75}
    monkeypatch.setattr(tr.model, "sample_latent_density", lambda d, n, **kw: (d, n, kw))
    assert tr.sample_latent_density("d", 5, seed=2) == ("d", 5, {"seed": 2})
