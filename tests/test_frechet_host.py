"""Host checks of the Frechet distance.  The float64 restatement the GPU tests of csrc/frechet.hip
are held to (tests/frechet_reference.py) reproduces what the reference's calculate_frechet_distance (scipy.linalg.sqrtm)
computed for the fixtures of tests/golden/frechet/ (recorded by tests/golden/make_golden_frechet.py; no test reads the
reference) by three routes; the spread of the independent routes sets each case's bar, which the GPU tests reuse;
frechet_distances keeps the metrics' contract on CPU models, where nothing reaches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

import frechet_reference as R
from conftest import GOLDEN_DIR, ROOT

SYMBOLS = ("mmvae_frechet_state_doubles", "mmvae_sym_eig_ws_doubles", "mmvae_frechet_ws_doubles",
           "mmvae_sym_eig_waves_per_pair", "mmvae_frechet_update", "mmvae_frechet_finish", "mmvae_f64_gemm", "mmvae_sym_eig",
           "mmvae_frechet_distance", "mmvae_digit_hidden")
fixture, case = R.fixture, R.case


# ---- 1. the restatement against the reference's recorded values ------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SMALL)
def test_inputs_are_the_documented_ones(name):
    c = case(name)
    fx = c["fx"]
    assert fx["X1"].dtype == np.float32 and np.array_equal(fx["X1"], c["X1"]) and np.array_equal(fx["X2"], c["X2"])
    iu = np.triu_indices(c["s1"].shape[0])
    assert np.array_equal(fx["mu1"], c["mu1"]) and np.array_equal(fx["mu2"], c["mu2"])
    assert np.array_equal(fx["sigma1_triu"], c["s1"][iu]) and np.array_equal(fx["sigma2_triu"], c["s2"][iu])
    _, F, N1, N2 = R.CASES[name]
    assert c["X1"].shape == (N1, F) and c["X2"].shape == (N2, F)
    if name == "d":
        assert np.all(c["s1"][R.CONSTANT_COLUMN] == 0.0) and np.all(c["s2"][:, R.CONSTANT_COLUMN] == 0.0)
        assert np.array_equal(c["s1"][R.DUPLICATED[0]], c["s1"][R.DUPLICATED[1]])
    if name == "c":
        assert np.linalg.matrix_rank(c["s1"]) == N1 - 1 < F


@pytest.mark.parametrize("name", list(R.CASES))
def test_three_routes_agree_with_the_recorded_value(name):
    c = case(name)
    print(f"{name}: recorded {c['recorded']:.15g}; eigh {R.rel(c['eigh'], c['recorded'], c['scale']):.2e}, nuclear norm "
          f"{R.rel(c['nuclear'], c['recorded'], c['scale']):.2e}, largest pairwise {c['spread']:.2e} -> bar {c['bar']:.2e}; "
          f"jacobi {R.rel(c['jacobi'], c['recorded'], c['scale']):.2e}")
    assert c["spread"] <= (1e-6 if name == "c" else 1e-11)      # rank-deficient: sqrt at eigenvalues of order eps lambda_max
    for other in ("recorded", "eigh", "nuclear"):
        assert R.rel(c["jacobi"], c[other], c["scale"]) <= c["bar"], other
    tr = float(c["fx"]["tr_covmean"])
    assert abs(c["tr_jacobi"] - tr) <= c["bar"] * (c["scale"] or max(abs(c["recorded"]), tr))
    if name == "e":
        assert abs(c["jacobi"]) <= c["bar"] * c["scale"]


@pytest.mark.parametrize("name", list(R.CASES))
def test_restated_jacobi_converges_within_the_cap(name):
    c = case(name)
    print(f"{name}: sweeps {c['sweeps']}")
    assert all(1 <= s <= 20 for s in c["sweeps"]), "replace the fixture: the restatement needs more than 20 sweeps"


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_restated_jacobi_is_an_eigendecomposition(name):
    S = case(name)["s1"]
    F = S.shape[0]
    lam, V, sweeps, counts = R.jacobi(S)
    ref = np.linalg.eigvalsh(S)
    bar = 4 * F * R.EPS
    errs = (np.abs(np.sort(lam) - ref).max() / ref.max(), np.abs(V.T @ V - np.eye(F)).max(),
            np.abs(S @ V - V * lam).max() / ref.max())
    print(f"{name}: values {errs[0]:.2e}, orthogonality {errs[1]:.2e}, residual {errs[2]:.2e} (bar {bar:.2e}); counted {counts}")
    assert max(errs) <= bar and counts[-1] == 0 and len(counts) == sweeps
    values_only = R.jacobi(S, vectors=False)
    assert np.array_equal(values_only[0], lam) and values_only[1] is None


def test_pairs_of_a_sweep_meet_once_and_steps_are_disjoint():
    """A check of the restatement's own ordering helper: it runs no library code.  The kernel's closed-form pair indices
    are tied to this helper on the GPU, where test_sym_eig compares the counted rotations of every sweep with the
    restatement's (tests/test_frechet_gpu.py)."""
    for n in (2, 6, 130):
        seen = set()
        for step in range(n - 1):
            p, q = R.pairs(n, step)
            assert len(set(p) | set(q)) == n and np.all(p < q)
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == n * (n - 1) // 2


def test_chan_merge_is_the_batch_covariance():
    c = case("b")
    st = R.chan_state(64)
    for lo, hi in ((0, 128), (128, 256), (256, 300)):
        R.chan_update(st, c["X1"][lo:hi])
    mu, sigma = R.chan_finish(st)
    assert st[0] == 300 and np.abs(mu - c["mu1"]).max() <= 1e-14 and np.abs(sigma - c["s1"]).max() <= 1e-13 * c["s1"].max()


def test_fixture_is_small_data():
    for name in R.CASES:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "frechet", name + ".npz")) <= 369060
    assert set(fixture("f")) == {"distance", "tr_covmean", "restated_distance", "restated_tr_covmean", "restated_sweeps"}


# ---- 2. the contract on CPU models ----------------------------------------------------------------------------------------------
def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


def _flat(x):
    return x.float().reshape(x.shape[0], -1)[:, :4]


def test_unimodal_vae_refuses_frechet_distances_by_name():
    from multimodal_vae_comparison_amd.models.vae import VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE)
    with pytest.raises(NotImplementedError) as e:
        vae.frechet_distances()
    assert "unimodal" in str(e.value) and "TorchMMVAE.frechet_distances" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="frechet_distances needs eval mode"):
        model.frechet_distances([cdsprites_batch(4, 6, seed=3)], {"mod_1": _flat})


def test_private_latents_have_no_joint_sample():
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch
    model = _model("dmvae", mods=[dict(m, private=4) for m in CD_MODS])
    with pytest.raises(NotImplementedError, match="frechet_distances"):
        model.frechet_distances([cdsprites_batch(4, 6, seed=3)], {"mod_1": _flat}, n_joint=8)


def test_argument_errors(monkeypatch):
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    with pytest.raises(ValueError, match="`batches` is empty"):
        model.frechet_distances([], {"mod_1": _flat})
    with pytest.raises(ValueError, match="without data"):
        model.frechet_distances([dict(batch, mod_2=dict(batch["mod_2"], data=None))], {"mod_1": _flat})
    with pytest.raises(ValueError, match="callables"):
        model.frechet_distances([batch], {"mod_9": _flat})
    with pytest.raises(ValueError, match="two rows"):
        model.frechet_distances([cdsprites_batch(1, 6, seed=3)], {"mod_1": _flat})
    with pytest.raises(ValueError, match="two rows"):
        model.frechet_distances([batch], {"mod_1": _flat}, n_joint=1)
    # an extractor whose F changes: the real rows of every batch are folded first, so the second call is the second
    # batch's; the fold itself is a kernel (refused on a CPU tensor) and is replaced by a recorder here
    folded = []
    monkeypatch.setattr(ops, "frechet_update", lambda state, f: folded.append(tuple(f.shape)))
    widths = iter((4, 5))
    with pytest.raises(ValueError, match="returned F = 5 after F = 4"):
        model.frechet_distances([batch, batch], {"mod_1": lambda x: x.float().reshape(x.shape[0], -1)[:, :next(widths)]})
    assert folded == [(4, 4)]
    with pytest.raises(ValueError, match=r"float \(rows, F\)"):
        model.frechet_distances([batch], {"mod_1": lambda x: x.reshape(-1)})
    # the ops' own checks name the limits before anything is launched
    with pytest.raises(ValueError, match="MI355X path"):
        ops.frechet_state(2049, "cpu")
    with pytest.raises(ValueError, match="MI355X path"):
        ops.sym_eig(torch.zeros(2049, 2049, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        ops.sym_eig(torch.zeros(4, 4))
    with pytest.raises(ValueError, match="not finite"):
        ops.sym_eig(torch.full((4, 4), float("nan"), dtype=torch.float64))
    with pytest.raises(ValueError, match="max_sweeps"):
        ops.sym_eig(torch.zeros(4, 4, dtype=torch.float64), max_sweeps=31)
    with pytest.raises(ValueError, match="n >= 2"):
        ops.frechet_moments(ops.frechet_state(3, "cpu"))
    z = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="mu2"):
        ops.frechet_distance(z, torch.zeros(4, 4, dtype=torch.float64), z[:3], torch.zeros(4, 4, dtype=torch.float64))


def test_update_checks_fire_before_a_launch():
    from multimodal_vae_comparison_amd import ops
    st = ops.frechet_state(4, "cpu")
    with pytest.raises(ValueError, match="the state holds floating"):
        ops.frechet_update(st, torch.zeros(3, 5))
    with pytest.raises(ValueError, match="not finite"):
        ops.frechet_update(st, torch.full((3, 4), float("inf")))
    assert ops.frechet_update(st, torch.zeros(0, 4)) is st and float(st.abs().max()) == 0.0
    for wrong in (torch.zeros(13), torch.zeros(12, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="frechet_state gives a contiguous float64 vector"):
            ops.frechet_update(wrong, torch.zeros(2, 3))
        with pytest.raises(ValueError, match="MI355X path"):
            ops.frechet_moments(wrong)


def test_a_failing_call_leaves_the_noise_setup_as_it_found_it():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    mine = model.eps_override = [torch.zeros(4, 8)]

    def broken(x):
        raise KeyError("the extractor fails inside the noise context")

    with pytest.raises(KeyError):
        model.frechet_distances([batch], {"mod_1": broken})
    assert model._eval_draws is False and torch.is_grad_enabled()
    assert model.eps_override is mine and len(mine) == 1
    with pytest.raises(ValueError, match="without data"):
        model.frechet_distances([dict(batch, mod_1=dict(batch["mod_1"], data=None))], {"mod_1": _flat})
    assert model._eval_draws is False and torch.is_grad_enabled() and model.eps_override is mine


# ---- 3. ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_header_and_the_ctypes_table():
    from multimodal_vae_comparison_amd import hipops
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES, f"{name} is not in the ctypes table"
    for macro, value in (("MMVAE_FRECHET_MAX_F", hipops.FRECHET_MAX_F), ("MMVAE_EIG_MAX_SWEEPS", hipops.EIG_MAX_SWEEPS)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    assert int(re.search(r"MMVAE_ERR_NO_CONVERGENCE = (\d+)", src).group(1)) == hipops.ERR_NO_CONVERGENCE
    assert R.MAX_SWEEPS == hipops.EIG_MAX_SWEEPS
    L = hipops.lib()
    for F in (1, 5, 130, 2048):
        eig = F * F + 2 * F + 64
        assert L.mmvae_frechet_state_doubles(F) == 1 + F + F * F
        assert L.mmvae_sym_eig_ws_doubles(F) == eig and L.mmvae_frechet_ws_doubles(F) == eig + 2 * F * F + 2 * F
    for F in (0, 2049):
        assert L.mmvae_frechet_state_doubles(F) == 0 and L.mmvae_sym_eig_ws_doubles(F) == 0
        assert L.mmvae_frechet_ws_doubles(F) == 0 and L.mmvae_sym_eig_waves_per_pair(F) == 0
    assert L.mmvae_sym_eig_waves_per_pair(256) == 1 and L.mmvae_sym_eig_waves_per_pair(257) == 4
