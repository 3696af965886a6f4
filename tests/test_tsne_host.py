"""Host checks of the latent analysis.  The float64 restatement the GPU tests of csrc/tsne.hip are
held to (tests/tsne_reference.py) reproduces what scikit-learn's exact t-SNE computed for the two fixtures of
tests/golden/tsne/ (recorded by tests/golden/make_golden_tsne.py; no test imports scikit-learn); the fixtures stay clear of
the two places where the kernels and the restatement may legitimately part -- the clamp of Q at eps and a perplexity
search that ends within rounding of its threshold; analyse_latents keeps the metrics' contract on CPU models, where
nothing reaches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

import tsne_reference as R
from conftest import GOLDEN_DIR, ROOT

CASES = ("a", "b")
SYMBOLS = ("mmvae_tsne_ld", "mmvae_tsne_ws_doubles", "mmvae_tsne_sqdist", "mmvae_tsne_joint_p", "mmvae_tsne_forces",
           "mmvae_tsne_run")


def fixture(name):
    z = np.load(os.path.join(GOLDEN_DIR, "tsne", name + ".npz"))
    return {k: z[k] for k in z.files}


_MEMO = {}


def searched(name):
    """(fixture, D2, conditional-P results, joint P float64) of a case, computed once"""
    if name not in _MEMO:
        fx = fixture(name)
        D2 = R.sqdist(fx["X"])
        cond = R.conditional_p(D2, float(fx["perplexity"]))
        C = cond[0]
        P = C + C.T
        P = np.maximum(P / max(P.sum(), R.EPS), R.EPS)
        np.fill_diagonal(P, 0.0)
        _MEMO[name] = (fx, D2, cond, P)
    return _MEMO[name]


# ---- 1. the restatement against scikit-learn's recorded outputs ---------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_inputs_are_the_documented_ones(name):
    fx = fixture(name)
    seed, N, D, C, perplexity = {"a": (11, 67, 8, 3, 10.0), "b": (12, 257, 20, 10, 30.0)}[name]
    X, labels = R.clustered(seed, N, D, C)
    assert fx["X"].dtype == np.float32 and np.array_equal(fx["X"], X) and np.array_equal(fx["labels"], labels)
    assert fx["Y0"].dtype == np.float32 and np.array_equal(fx["Y0"], R.default_init(N, 123))
    assert float(fx["perplexity"]) == perplexity


@pytest.mark.parametrize("name", CASES)
def test_joint_probabilities_are_scikit_learns(name):
    fx, _, _, P = searched(name)
    if name == "a":
        N = P.shape[0]
        assert np.array_equal(fx["P_full"][np.triu_indices(N, 1)], fx["P_condensed"])
        got, ref = P, fx["P_full"]
    else:
        got, ref = P[fx["P_rows_index"]], fx["P_rows"]
    err = np.abs(got - ref).max() / ref.max()
    print(f"{name}: P deviates by {err:.2e} of its maximum")
    assert err <= 1e-6
    assert np.abs(P.sum(1) - fx["P_rowsum"]).max() <= 1e-6 * fx["P_rowsum"].max()
    assert abs(P.sum() - 1.0) <= 1e-9 and np.array_equal(P, P.T)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("ex", [1, 12])
def test_objective_and_gradient_are_scikit_learns(name, ex):
    fx, _, _, P = searched(name)
    g, kl, _, _ = R.forces(fx["Y0"], P, float(ex))
    ref = fx[f"grad_ex{ex}"]
    gerr, kerr = np.abs(g - ref).max() / np.abs(ref).max(), abs(kl - fx[f"kl_ex{ex}"]) / fx[f"kl_ex{ex}"]
    print(f"{name} ex {ex}: gradient {gerr:.2e} of its maximum, KL {kerr:.2e} relative")
    assert gerr <= 1e-6 and kerr <= 1e-8


def test_recorded_run_and_the_tests_own_scores():
    """case B's full scikit-learn run left a small objective and a high trustworthiness; the tests' numpy scores give
    the trivial answers on trivial inputs (an embedding equal to the data is perfectly trustworthy)"""
    fx = fixture("b")
    assert 0.98 < float(fx["final_trustworthiness"]) <= 1.0 and 0.0 < float(fx["final_kl"]) < 0.1
    assert R.trustworthiness(fx["X"], fx["X"], 5) == 1.0
    shuffled = fx["X"][np.random.RandomState(0).permutation(len(fx["X"]))]
    assert R.trustworthiness(fx["X"], shuffled, 5) < 0.7
    assert R.neighbour_purity(fx["X"], fx["labels"], 5) > 0.9 > R.neighbour_purity(shuffled, fx["labels"], 5)


def test_fixture_is_small_data():
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "tsne", name + ".npz")) <= 369060


# ---- 2. the fixtures stay clear of the edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_no_pair_reaches_the_clamp_of_q(name):
    """g = 4 (ex attr - rep / Z), the form the kernels compute, is the definition's sum wherever w_ij / Z >= eps"""
    fx, _, _, P = searched(name)
    P32 = P.astype(np.float32)
    _, _, _, wmin = R.run(R.fresh(fx["Y0"]), P32, 0, 400, R.default_lr(P.shape[0]), track_w=True)
    wmin = min(wmin, R.forces(fx["Y0"], P32, 1.0)[3])
    print(f"{name}: least w_ij / Z over 400 iterations = {wmin:.3e} = {wmin / R.EPS:.3e} eps")
    assert wmin >= R.EPS


@pytest.mark.parametrize("name", CASES)
def test_no_search_ends_within_rounding_of_its_threshold(name):
    _, _, (_, _, steps, traces, zero), _ = searched(name)
    margin = min(abs(abs(t) - 1e-5) for tr in traces for t in tr[-2:])
    print(f"{name}: closest |H - log perplexity| to 1e-5 at a last or last-but-one step: {margin:.3e}; "
          f"most steps {steps.max()}")
    assert margin > 1e-9 and steps.max() < 100 and not zero


def test_float32_switch_runs_in_float32():
    fx, _, _, P = searched("a")
    st64, _, _, _ = R.run(R.fresh(fx["Y0"]), P, 0, 3, 50.0)
    st32, _, _, _ = R.run(R.fresh(fx["Y0"], np.float32), P, 0, 3, 50.0, dtype=np.float32)
    assert st64[0].dtype == np.float64 and st32[0].dtype == np.float32
    d = np.abs(st32[0] - st64[0]).max() / np.abs(st64[0]).max()
    assert 0.0 < d < 1e-4


# ---- 3. the contract on CPU models ----------------------------------------------------------------------------------------------
def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


def test_unimodal_vae_refuses_analyse_latents_by_name():
    from multimodal_vae_comparison_amd.models.vae import VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE)
    with pytest.raises(NotImplementedError) as e:
        vae.analyse_latents()
    assert "unimodal" in str(e.value) and "TorchMMVAE.analyse_latents" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="analyse_latents needs eval mode"):
        model.analyse_latents([cdsprites_batch(4, 6, seed=3)])


def test_perplexity_must_stay_below_the_point_count():
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):      # 2 modalities x 4 samples
        model.analyse_latents([cdsprites_batch(4, 6, seed=3)], perplexity=8.0)
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        ops.tsne_embed(torch.zeros(30, 4), perplexity=30.0)
    with pytest.raises(ValueError, match="max_iter"):
        ops.tsne_embed(torch.zeros(30, 4), perplexity=5.0, max_iter=249)
    with pytest.raises(ValueError, match="not finite"):
        ops.tsne_embed(torch.full((30, 4), float("nan")), perplexity=5.0)
    for shape in ((3, 4), (16385, 2), (30, 257)):
        with pytest.raises(ValueError, match="MI355X path"):
            ops.tsne_embed(torch.zeros(*shape), perplexity=2.0)


def test_a_failing_call_leaves_the_noise_setup_as_it_found_it():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    batch["mod_1"] = dict(batch["mod_1"], data=None)
    mine = model.eps_override = [torch.zeros(4, 8)]
    with pytest.raises(ValueError, match="every batch"):
        model.analyse_latents([batch], perplexity=2.0)
    assert model._eval_draws is False and torch.is_grad_enabled()
    assert model.eps_override is mine and len(mine) == 1


def test_default_init_is_scikit_learns_draw():
    from multimodal_vae_comparison_amd import ops
    got = ops.tsne_default_init(67, 123)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), fixture("a")["Y0"])
    assert ops.tsne_default_lr(257) == 50.0 and ops.tsne_default_lr(4800) == 100.0


# ---- 4. ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_header_and_the_ctypes_table():
    from multimodal_vae_comparison_amd import hipops
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES, f"{name} is not in the ctypes table"
    for macro, value in (("MMVAE_TSNE_MAX_POINTS", hipops.TSNE_MAX_POINTS), ("MMVAE_TSNE_MAX_DIM", hipops.TSNE_MAX_DIM),
                         ("MMVAE_TSNE_MIN_POINTS", hipops.TSNE_MIN_POINTS)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    L = hipops.lib()
    assert L.mmvae_tsne_ld(257) == 260 and L.mmvae_tsne_ld(3) == 0 and L.mmvae_tsne_ld(16385) == 0
    assert L.mmvae_tsne_ws_doubles(67) == 67 * 8
