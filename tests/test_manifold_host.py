"""Host checks of precision, recall, density and coverage.  The float64 restatement the GPU tests of
csrc/manifold.hip are held to (tests/manifold_reference.py: direct differences, no Gram product) against a case worked by
hand and against the estimates' identities; manifold_metrics keeps the metrics' contract on CPU models, where nothing
reaches a kernel; the ops refuse what is outside the limits before any launch."""
import os
import re

import numpy as np
import pytest
import torch

import manifold_reference as R
from conftest import ROOT

SYMBOLS = ("mmvae_manifold_chunks", "mmvae_manifold_ws_doubles", "mmvae_manifold_sqnorms", "mmvae_manifold_radii",
           "mmvae_manifold_cross")


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------
def test_integer_case_by_hand():
    """k = 1.  Real: the square (0,0) (2,0) (0,2) (2,2) has its nearest corner at d^2 = 4, (5,5) is 18 from (2,2).  Generated:
    (1,0) and (2,0) are 1 apart, (4,2) is 8 from (2,0), (9,9) is 74 from (4,2), (0,4) is 17 from (1,0).
    (1,0) lies in the spheres of (0,0), (2,0); (2,0) -- a duplicate of a real row -- in those of (0,0) ON the sphere,
    (2,0), (2,2) ON the sphere; (4,2) in those of (2,2) ON the sphere and (5,5); (9,9) in none; (0,4) in that of (0,2) ON
    the sphere: hits 2, 3, 2, 0, 1 -> precision 4/5, density 8/5.  Every real row is in some generated sphere (recall 1) and
    has a generated row within its own radius (coverage 1; (5,5): 10 <= 18)."""
    o = R.prdc(R.INT_REAL, R.INT_FAKE, 1)
    assert o["rad2_real"].tolist() == [4, 4, 4, 4, 18] and o["rad2_fake"].tolist() == [1, 1, 8, 74, 17]
    assert o["hit_real"].tolist() == [2, 3, 2, 0, 1] and o["hit_fake"].tolist() == [2, 3, 1, 2, 1]
    assert o["near_real"].tolist() == [1, 0, 4, 4, 10]
    assert [o[n] for n in R.SCALARS] == [0.8, 1.0, 1.6, 1.0]
    assert o["margin"] == 0.0      # distances exactly on a sphere: `<` in place of `<=` gives another result
    D = R.sqdist(R.INT_FAKE, R.INT_REAL)
    strict = (D < o["rad2_real"][None, :]).sum(1)
    assert strict.tolist() == [2, 1, 1, 0, 0] and int((strict > 0).sum()) / 5 == 0.6


def test_identities():
    Rr, G, k, o = R.case(1)
    back = R.prdc(G, Rr, k)
    assert o["precision"] == back["recall"] and o["recall"] == back["precision"]
    assert np.array_equal(o["hit_real"], back["hit_fake"]) and np.array_equal(o["rad2_real"], back["rad2_fake"])
    same = R.prdc(Rr, Rr, k)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["density"] >= 1.0
    far = R.prdc(Rr, G + np.float32(1e3), k)
    assert [far[n] for n in R.SCALARS] == [0.0, 0.0, 0.0, 0.0]


def test_a_duplicated_row_is_a_neighbour_at_zero():
    X = np.array(R.case(0)[0])
    X[4] = X[1]
    rad = R.radii(X, 1)
    assert rad[1] == 0.0 and rad[4] == 0.0 and np.all(rad[[0, 2, 3, 5, 6, 7, 8]] > 0.0)
    assert np.all(R.radii(X, 2) > 0.0)


def test_generator_is_the_documented_one():
    F = 5
    W = np.random.RandomState(7).standard_normal((F, F)) / np.sqrt(F)
    X = np.maximum((0.15 + 0.9 * np.random.RandomState(2).standard_normal((6, F))) @ W + 0.25, 0.0).astype(np.float32)
    Rr, G, k, _ = R.case(0)
    assert np.array_equal(G, X) and G.dtype == np.float32 and Rr.shape == (9, 5) and k == 1
    assert np.array_equal(Rr, R.features(9, 5, 1)) and (Rr == 0).any() and (Rr > 0).any()


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_margin_makes_exact_counts_a_fair_demand(i):
    """what the GPU tests assert again before they ask for exact equality: no compared distance is within 10^3 rounding
    bars of its radius, and the scalars are not trivially 0 or 1"""
    _, _, _, o = R.case(i)
    b = R.bar(R.SHAPES[i][2], o["scale"])
    print(f"{R.SHAPES[i]}: " + ", ".join(f"{n} {o[n]:.4f}" for n in R.SCALARS) + f"; margin {o['margin'] / b:.3g} bars")
    assert o["margin"] >= 1e3 * b
    assert all(0.0 < o[n] < 1.0 or n == "density" or (n == "coverage" and i == 2) for n in R.SCALARS) and o["density"] > 0.0


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


def test_unimodal_vae_refuses_manifold_metrics_by_name():
    from multimodal_vae_comparison_amd.models.vae import VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE)
    with pytest.raises(NotImplementedError) as e:
        vae.manifold_metrics()
    assert "unimodal" in str(e.value) and "TorchMMVAE.manifold_metrics" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="manifold_metrics needs eval mode"):
        model.manifold_metrics([cdsprites_batch(4, 6, seed=3)], {"mod_1": _flat}, k=1)


def test_private_latents_have_no_joint_sample():
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch
    model = _model("dmvae", mods=[dict(m, private=4) for m in CD_MODS])
    with pytest.raises(NotImplementedError, match="manifold_metrics"):
        model.manifold_metrics([cdsprites_batch(4, 6, seed=3)], {"mod_1": _flat}, k=1, n_joint=8)


def test_argument_errors_come_before_the_first_forward(monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    calls = []
    forward = model.forward
    monkeypatch.setattr(model, "forward", lambda *a, **kw: calls.append(1) or forward(*a, **kw))
    with pytest.raises(ValueError, match="manifold_metrics: `batches` is empty"):
        model.manifold_metrics([], {"mod_1": _flat})
    with pytest.raises(ValueError, match="manifold_metrics: .*without data"):
        model.manifold_metrics([dict(batch, mod_2=dict(batch["mod_2"], data=None))], {"mod_1": _flat}, k=1)
    with pytest.raises(ValueError, match="manifold_metrics: .*callables"):
        model.manifold_metrics([batch], {"mod_9": _flat}, k=1)
    with pytest.raises(ValueError, match=r"manifold_metrics: 4 real rows.*k \+ 1 = 5 rows"):
        model.manifold_metrics([batch], {"mod_1": _flat}, k=4)
    with pytest.raises(ValueError, match="manifold_metrics: 8 real rows, n_joint = 3"):
        model.manifold_metrics([batch, batch], {"mod_1": _flat}, k=3, n_joint=3)
    for k in (0, 17):
        with pytest.raises(ValueError, match=f"manifold_metrics: k = {k} neighbours"):
            model.manifold_metrics([batch] * 8, {"mod_1": _flat}, k=k)
    big = dict(batch, mod_1=dict(batch["mod_1"], data=torch.zeros(1, 3, 64, 64).expand(16385, 3, 64, 64)))
    with pytest.raises(ValueError, match="manifold_metrics: 16385 real rows"):
        model.manifold_metrics([big], {"mod_1": _flat}, k=1)
    assert not calls


def test_extractor_misuse():
    """the real rows of every batch go through the extractor before the first forward(): the second call is the second
    batch's"""
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    widths = iter((4, 5))
    with pytest.raises(ValueError, match="manifold_metrics: the extractor of 'mod_1' returned F = 5 after F = 4"):
        model.manifold_metrics([batch, batch], {"mod_1": lambda x: x.float().reshape(x.shape[0], -1)[:, :next(widths)]}, k=1)
    with pytest.raises(ValueError, match=r"manifold_metrics: the extractor of 'mod_1' must return float \(rows, F\)"):
        model.manifold_metrics([batch], {"mod_1": lambda x: x.reshape(-1)}, k=1)
    assert model._eval_draws is False and model.eps_override is None and torch.is_grad_enabled()


def test_a_failing_call_leaves_the_noise_setup_as_it_found_it():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    mine = model.eps_override = [torch.zeros(4, 8)]

    def broken(x):
        raise KeyError("the extractor fails inside the noise context")

    with pytest.raises(KeyError):
        model.manifold_metrics([batch], {"mod_1": broken}, k=1)
    assert model._eval_draws is False and torch.is_grad_enabled()
    assert model.eps_override is mine and len(mine) == 1


def test_ops_refuse_before_a_launch():
    from multimodal_vae_comparison_amd import ops
    x = torch.ones(6, 4)
    for k in (0, 17):
        with pytest.raises(ValueError, match="manifold_radii: k ="):
            ops.manifold_radii(x, k)
        with pytest.raises(ValueError, match="manifold_prdc: k ="):
            ops.manifold_prdc(x, x, k=k)
    with pytest.raises(ValueError, match="manifold_radii: X has 6 rows"):
        ops.manifold_radii(x, 6)
    with pytest.raises(ValueError, match="manifold_radii: X has 16385 rows"):
        ops.manifold_radii(torch.ones(16385, 2), 1)
    with pytest.raises(ValueError, match="manifold_radii: X has F = 2049"):
        ops.manifold_radii(torch.ones(6, 2049), 1)
    with pytest.raises(ValueError, match=r"manifold_radii: X is \(6,\)"):
        ops.manifold_radii(torch.ones(6), 1)
    with pytest.raises(ValueError, match="manifold_radii: X is .*int64"):
        ops.manifold_radii(torch.ones(6, 4, dtype=torch.int64), 1)
    with pytest.raises(ValueError, match="manifold_radii: X holds values that are not finite"):
        ops.manifold_radii(torch.full((6, 4), float("nan")), 1)
    with pytest.raises(ValueError, match="manifold_radii: chunks = -1"):
        ops.manifold_radii(x, 1, chunks=-1)
    with pytest.raises(ValueError, match="manifold_sqnorms: X has F = 2049"):
        ops.manifold_sqnorms(torch.ones(6, 2049))
    rad = torch.ones(6, dtype=torch.float64)
    with pytest.raises(ValueError, match="manifold_cross: queries have F = 3 features, the manifold F = 4"):
        ops.manifold_cross(torch.ones(5, 3), x, rad)
    with pytest.raises(ValueError, match="manifold_cross: rad2 is .*float32"):
        ops.manifold_cross(x, x, rad.float())
    with pytest.raises(ValueError, match=r"manifold_cross: rad2 is \(5,\)"):
        ops.manifold_cross(x, x, rad[:5])
    with pytest.raises(ValueError, match="manifold_cross: rad2 is on meta, the manifold rows on cpu"):
        ops.manifold_cross(x, x, rad.to("meta"))
    with pytest.raises(ValueError, match="manifold_cross: manifold has 16385 rows"):
        ops.manifold_cross(x, torch.ones(16385, 4), rad)
    with pytest.raises(ValueError, match="manifold_cross: queries holds values that are not finite"):
        ops.manifold_cross(torch.full((6, 4), float("inf")), x, rad)
    with pytest.raises(ValueError, match="manifold_prdc: fake has 5 rows"):
        ops.manifold_prdc(x, torch.ones(5, 4), k=5)
    with pytest.raises(ValueError, match="manifold_prdc: real has F = 4 features, fake F = 3"):
        ops.manifold_prdc(x, torch.ones(6, 3), k=2)


# ---- 3. ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_header_and_the_ctypes_table():
    from multimodal_vae_comparison_amd import hipops
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES, f"{name} is not in the ctypes table"
    for macro, value in (("MMVAE_MANIFOLD_MAX_ROWS", hipops.MANIFOLD_MAX_ROWS), ("MMVAE_MANIFOLD_MAX_K", hipops.MANIFOLD_MAX_K)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    L = hipops.lib()
    # the default plan: min(ceil(512 / row tiles), ceil(column tiles / 4)) chunks, none of them empty
    assert L.mmvae_manifold_chunks(10000, 10000) == 4 and L.mmvae_manifold_chunks(9, 6) == 1
    assert L.mmvae_manifold_chunks(900, 1100) == 5 and L.mmvae_manifold_chunks(300, 300) == 2
    assert L.mmvae_manifold_chunks(16384, 16384) == 2 and L.mmvae_manifold_chunks(64, 16384) == 64
    assert L.mmvae_manifold_ws_doubles(10000, 10000, 5, 0) == 4 * 10000 * 5
    assert L.mmvae_manifold_ws_doubles(900, 1100, 1, 0) == 5 * 900 * 2
    assert L.mmvae_manifold_ws_doubles(300, 300, 8, 1) == 300 * 8 and L.mmvae_manifold_ws_doubles(300, 300, 8, 99) == 5 * 300 * 8
    assert L.mmvae_manifold_ws_doubles(300, 300, 8, 4) == 3 * 300 * 8      # 5 tiles in chunks of 2: the fourth would be empty
    for rows, cols, k, chunks in ((0, 5, 1, 0), (5, 0, 1, 0), (16385, 5, 1, 0), (5, 16385, 1, 0), (5, 5, 0, 0), (5, 5, 17, 0),
                                  (5, 5, 1, -1)):
        assert L.mmvae_manifold_ws_doubles(rows, cols, k, chunks) == 0
    assert L.mmvae_manifold_chunks(0, 5) == 0 and L.mmvae_manifold_chunks(5, 16385) == 0


# ---- 4. the routing of the sets, on a CPU model with a scripted forward() ------------------------------------------------------
def test_sets_are_routed_to_their_keys_and_log_tags(monkeypatch):
    """forward() is scripted (on a CPU model the real one would reach a kernel) to return, per call, rows that depend on
    which modalities it was given and on the batch; ops.manifold_prdc is the restatement.  Every set then has its own four
    numbers, so a set filed under another key, a swapped pair or a permuted log tag shows."""
    import types
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    B, K, names = 4, 2, ("mod_1", "mod_2")
    cfg, dims = config_from_mods("mopoe", CD_MODS, 8, batch_size=B)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cpu")
    model = tr.model
    model.eval()
    rng = np.random.RandomState(5)
    batches = []
    for i in range(2):
        b = cdsprites_batch(B, 6, seed=3 + i)
        for m in names:      # the first four values of a row are its features
            b[m]["data"].reshape(B, -1)[:, :4] = torch.from_numpy(rng.standard_normal((B, 4)).astype(np.float32))
        batches.append(b)
    shift = {names: 0.2, ("mod_1",): 0.5, ("mod_2",): 0.9}
    made, order = {}, []

    def forward(batch):
        given = tuple(m for m in names if batch[m]["data"] is not None)
        i = next(n for n, b in enumerate(batches) if all(batch[m]["masks"] is b[m]["masks"] for m in names))
        order.append((i, given))
        out = {}
        for m in names:      # B + 2 rows: the metric keeps the first B
            loc = torch.zeros((B + 2,) + tuple(batches[i][m]["data"].shape[1:]))
            loc.reshape(B + 2, -1)[:, :4] = torch.from_numpy((shift[given] * (1 + names.index(m))
                                                              + 0.7 * rng.standard_normal((B + 2, 4))).astype(np.float32))
            made[(i, given, m)] = loc
            out[m] = types.SimpleNamespace(decoder_dist=types.SimpleNamespace(loc=loc))
        return types.SimpleNamespace(mods=out)

    def restated(real, fake, k=5):
        o = R.prdc(real.numpy(), fake.numpy(), k)
        return {n: o[n] for n in R.SCALARS}

    monkeypatch.setattr(model, "forward", forward)
    monkeypatch.setattr(ops, "manifold_prdc", restated)
    res = tr.manifold_metrics(batches, {"mod_1": _flat, "mod_2": _flat}, k=K)
    assert order == [(0, names), (0, ("mod_1",)), (0, ("mod_2",)), (1, names), (1, ("mod_1",)), (1, ("mod_2",))]
    logged, fours = {}, []
    for m, other in (("mod_1", "mod_2"), ("mod_2", "mod_1")):
        real = np.concatenate([_flat(b[m]["data"]).numpy() for b in batches])
        sets = {"recon": names, "cross": (other,)}
        want = {}
        for key, given in sets.items():
            gen = np.concatenate([_flat(made[(i, given, m)]).numpy()[:B] for i in range(2)])
            o = R.prdc(real, gen, K)
            want[key] = {n: o[n] for n in R.SCALARS}
            fours.append(tuple(want[key].values()))
        r = res[m]
        assert (r["n"], r["F"], r["k"], r["joint"]) == (2 * B, 4, K, None) and set(r["cross"]) == {other}
        assert r["recon"] == want["recon"] and r["cross"][other] == want["cross"]
        for n in R.SCALARS:
            logged[f"test_{n}_{m}_recon"] = want["recon"][n]
            logged[f"test_{n}_{m}_from_{other}"] = want["cross"][n]
    assert len(set(fours)) == 4 and all(any(0.0 < v < 1.0 for v in four) for four in fours), fours
    assert {k: float(v) for k, v in tr.logged.items() if k.startswith("test_")} == logged
