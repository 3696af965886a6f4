"""Host tests of the sliced Wasserstein distances and marginal KS tests (csrc/swd.hip): the numpy
longdouble restatement of tests/swd_reference.py against scipy, against the brute-force W_p of repeated samples and against a
case worked by hand; the float64 restatement inside the bounds the GPU tests use (so they are not vacuous) and far enough
outside them when an error is seeded; ops.ks_p_value against scipy.special.kolmogorov; the recipe of ops.swd_draw; the ABI;
every refusal before a launch; the two model methods on scripted posteriors."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import swd_reference as R
from conftest import ROOT

SYMBOLS = ("mmvae_swd_ws_doubles", "mmvae_swd_slices")
STARRED = ((7, 5, 3, 4), (64, 64, 8, 16), (257, 130, 33, 16), (300, 211, 256, 8), (1000, 1024, 5, 32))


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 5, 3, 4), (65, 63, 8, 16), (257, 130, 33, 16), (1, 1, 1, 1), (1, 9, 2, 3)])
def test_restatement_against_scipy(shape):
    from scipy import stats
    c = R.case(*shape)
    px, py = R.project(c.X, c.dirs, np.float64), R.project(c.Y, c.dirs, np.float64)
    for l in range(c.L):
        w1 = stats.wasserstein_distance(px[l], py[l])
        assert abs(w1 - float(c.ref["w"][l, 0])) <= 1e-13 * max(w1, 1e-300) + 2 * c.e[l], (shape, l)
        d = stats.ks_2samp(px[l], py[l]).statistic
        assert abs(d - c.ref["ks"][l] / (c.n_x * c.n_y)) <= 1e-14, (shape, l)


@pytest.mark.parametrize("sizes", [(7, 5), (5, 7), (1, 4), (13, 8), (64, 27), (9, 9)])
def test_restatement_against_repeated_samples(sizes):
    """W_p of two empirical measures = W_p of the two lists of n_x n_y values with every x repeated n_y times and every y
    n_x times: sorted, the mean of |difference|^p"""
    n_x, n_y = sizes
    rs = np.random.RandomState(n_x * 100 + n_y)
    x, y = np.sort(rs.standard_normal(n_x)), np.sort(0.5 * rs.standard_normal(n_y) + 1.0)
    w1, w2 = R.grid_walk(x, y)
    d = np.abs(np.sort(np.repeat(x, n_y)).astype(R.LD) - np.sort(np.repeat(y, n_x)).astype(R.LD))
    assert abs(w1 - d.mean()) <= 1e-17 * float(d.mean()) * len(d) and abs(w2 - (d * d).mean()) <= 1e-17 * float((d * d).mean()) * len(d)
    f1, f2 = R.grid_walk(x, y, np.float64)
    assert abs(f1 - float(w1)) <= (n_x + n_y + 8) * R.U * float(w1) and abs(f2 - float(w2)) <= (n_x + n_y + 8) * R.U * float(w2)


def test_case_by_hand():
    """X = {0, 1}, Y = {0, 1, 2} on one axis.  The grid of sixths: x covers [0,3) [3,6), y covers [0,2) [2,4) [4,6); cells
    (0,0) 2, (0,1) 1, (1,1) 1, (1,2) 2 with |d| = 0, 1, 0, 1: W_1 = 3 / 6, W_2^2 = 3 / 6.  CDFs at 0, 1, 2: 1/2, 1, 1 against
    1/3, 2/3, 1: numerators |3 - 2|, |6 - 4|, 0"""
    out = R.restate(np.array([[0.0], [1.0]], np.float32), np.array([[0.0], [1.0], [2.0]], np.float32))
    assert out["w"].tolist() == [[0.5, 0.5]] and out["ks"].tolist() == [2]
    out = R.restate(np.array([[1.0], [0.0]], np.float32), np.array([[1.0], [0.0]], np.float32))
    assert out["w"].tolist() == [[0.0, 0.0]] and out["ks"].tolist() == [0]
    # -0.0 ties with +0.0
    assert R.ks_numerator(np.array([-0.0, 0.0]), np.array([0.0, -0.0])) == 0


@pytest.mark.parametrize("shape", STARRED + ((65, 63, 8, 16), (1, 1, 1, 1)))
def test_float64_restatement_sits_inside_the_bounds(shape):
    """the bounds hold for plain float64 numpy (a BLAS product, numpy's pairwise sums) and are not vacuous: they are a few
    hundred roundings wide at the most, and the pooled projections are far enough apart for ks to be compared exactly"""
    for axis in (False, True):
        if axis and shape[2] > 1024:
            continue
        c = R.case(*shape, axis=axis)
        assert c.gap_ok, (shape, axis, float((c.gaps / np.maximum(c.e, 1e-300)).min()))
        out = R.restate(c.X, c.Y, c.dirs, np.float64)
        f1, f2 = c.held(out["w"], out["ks"])
        w1, w2 = c.ref["w"][:, 0].astype(np.float64), c.ref["w"][:, 1].astype(np.float64)
        print(f"{shape} axis {axis}: float64 numpy at {f1:.3g} / {f2:.3g} of the bounds; smallest gap "
              f"{float((c.gaps / np.maximum(c.e, 1e-300)).min()):.3g} projection bounds")
        if shape[0] > 1:
            assert np.all(c.b1 <= 1e-11 * w1) and np.all(c.b2 <= 1e-11 * w2)
        if axis:
            assert np.all(c.e == 0) and np.all(c.b1 == (c.n_x + c.n_y + 8) * R.U * w1)


@pytest.mark.parametrize("axis", [True, False])
def test_ties_cases(axis):
    c = R.ties_case(axis)
    assert c.gap_ok
    pooled = np.concatenate([c.ref["px"], c.ref["py"]], axis=1)
    assert all(len(np.unique(p)) < len(p) for p in pooled), "every direction holds exact ties"
    if axis:
        assert c.ref["w"][5].tolist() == [0.0, 0.0] and c.ref["ks"][5] == 0      # the constant column
        assert np.any(np.signbit(c.X) & (c.X == 0)) and np.any(~np.signbit(c.X) & (c.X == 0))
        same = R.restate(c.X, c.X, None)
        assert not same["w"].any() and not same["ks"].any()
    out = R.restate(c.X, c.Y, c.dirs, np.float64)
    c.held(out["w"], out["ks"])


def test_seeded_errors_leave_the_bounds():
    c = R.case(257, 130, 33, 16)
    px, py = c.ref["px"], c.ref["py"]
    # equal weights instead of the grid of 1 / N (the first n_y quantiles paired)
    wrong = np.array([[np.abs(px[l][:130] - py[l]).mean(), (np.abs(px[l][:130] - py[l]) ** 2).mean()] for l in range(c.L)])
    e1, e2 = c.errors(wrong)
    assert np.all(e1 > c.b1) and np.all(e2 > c.b2)
    # W_2 in place of W_2^2; a count that is strict on one side (#{x <= t} against #{y < t}) moves ks under ties
    e1, e2 = c.errors(np.stack([c.ref["w"][:, 0], np.sqrt(c.ref["w"][:, 1])], 1))
    assert not np.any(e1 > c.b1) and np.all(e2 > c.b2)
    t = R.ties_case(True)
    strict = [int(np.abs(t.n_y * np.searchsorted(t.ref["px"][l], np.unique(t.ref["px"][l]), "right") -
                         t.n_x * np.searchsorted(t.ref["py"][l], np.unique(t.ref["px"][l]), "left")).max()) for l in range(5)]
    assert all(a != b for a, b in zip(strict, t.ref["ks"][:5].tolist()))
    # fp32 projections miss the bound by orders of magnitude
    p32 = lambda A: (np.asarray(c.dirs, np.float32) @ A.T).astype(np.float64)
    w = np.array([R.grid_walk(np.sort(p32(c.X)[l]), np.sort(p32(c.Y)[l]), np.float64) for l in range(c.L)], np.float64)
    e1, e2 = c.errors(w)
    assert np.all(e1 > 100 * c.b1)


# ---- 2. the p-value and the draw ----------------------------------------------------------------------------------------------------
def test_ks_p_value_against_scipy():
    from scipy import special
    from multimodal_vae_comparison_amd import ops
    for n_x, n_y in ((6, 4), (64, 64), (1000, 1024), (8192, 8191), (1, 1)):
        d = np.concatenate([[0.0, 1.0 / (n_x * n_y), 1.0], np.linspace(0.0, 1.0, 41)])
        root = np.sqrt(n_x * n_y / (n_x + n_y))
        want = special.kolmogorov((root + 0.12 + 0.11 / root) * d)
        got = ops.ks_p_value(d, n_x, n_y)
        assert got.dtype == np.float64 and got.shape == d.shape and np.all((got >= 0) & (got <= 1))
        assert np.allclose(got, want, rtol=1e-12, atol=1e-15), (n_x, n_y, np.abs(got - want).max())
        assert got[0] == 1.0 and ops.ks_p_value(0.0, n_x, n_y) == 1.0 and isinstance(ops.ks_p_value(0.3, n_x, n_y), float)
        assert np.array_equal(ops.ks_p_value(torch.from_numpy(d), n_x, n_y), got)
    assert ops.ks_p_value(1.0, 1000, 1000) < 1e-300
    for bad in ((-0.1, 3, 3), (1.5, 3, 3), (0.5, 0, 3)):
        with pytest.raises(ValueError, match="ks_p_value"):
            ops.ks_p_value(*bad)
    assert "Stephens" in ops.ks_p_value.__doc__


def test_draw_is_the_documented_recipe():
    from multimodal_vae_comparison_amd import ops
    for F, L, seed in ((3, 4, 0), (1, 1, 5), (256, 8, 0), (12288, 3, 7)):
        got = ops.swd_draw(F, L, seed)
        g = np.random.RandomState(seed).standard_normal((L, F))
        want = g / np.sqrt((g * g).sum(1, keepdims=True))
        assert got.dtype == np.float64 and got.shape == (L, F) and np.array_equal(got, want) and np.array_equal(got, R.draw(F, L, seed))
        assert np.all(np.abs((got.astype(R.LD) ** 2).sum(1) - 1) <= 4 * 2.0 ** -52)
        assert np.array_equal(ops.swd_draw(F, L, seed), got) and not np.array_equal(ops.swd_draw(F, L, seed + 1), got)
    assert "RandomState(seed)" in ops.swd_draw.__doc__ and "standard_normal((L, F))" in ops.swd_draw.__doc__


# ---- 3. the ABI --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_limits():
    from multimodal_vae_comparison_amd import hipops, ops
    from multimodal_vae_comparison_amd.models.vae import MIXER_METRICS
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES and hasattr(hipops.lib(), name)
    for macro, value in (("MMVAE_SWD_MAX_ROWS", hipops.SWD_MAX_ROWS), ("MMVAE_SWD_MAX_F", hipops.SWD_MAX_F),
                         ("MMVAE_SWD_MAX_DIRECTIONS", hipops.SWD_MAX_DIRECTIONS)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value, macro
    assert (hipops.SWD_MAX_ROWS, hipops.SWD_MAX_F, hipops.SWD_MAX_DIRECTIONS) == (8192, 16384, 1024)
    assert "latent_transport" in MIXER_METRICS and "sliced_distances" in MIXER_METRICS
    assert "swd.hip" in open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "Makefile")).read()
    for name in ("swd_draw", "swd_slices", "ks_p_value", "sliced_wasserstein", "marginal_tests"):
        assert callable(getattr(ops, name))
    assert "from .metrics.swd import *" in open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "ops.py")).read()


def test_pure_queries_and_refusals_of_the_entry_point_run_without_gpu():
    from multimodal_vae_comparison_amd import hipops as H
    L = H.lib()
    ws = L.mmvae_swd_ws_doubles
    assert ws(7, 5, 3, 4) == 4 * 12 and ws(8192, 8192, 16384, 1024) == 1024 * 16384 and ws(1, 1, 1, 1) == 2
    assert ws(0, 5, 3, 4) == ws(7, 0, 3, 4) == ws(8193, 5, 3, 4) == ws(7, 8193, 3, 4) == 0
    assert ws(7, 5, 0, 4) == ws(7, 5, 16385, 4) == ws(7, 5, 3, 0) == ws(7, 5, 3, 1025) == 0
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, H.c_p)
    base = dict(X=p, Y=p, dirs=p, ws=p, w=p, ks=p, n_x=8, n_y=8, F=4, L=2, stream=None)

    def call(**k):
        return L.mmvae_swd_slices(*{**base, **k}.values())
    for bad in (dict(n_x=0), dict(n_y=0), dict(n_x=8193), dict(n_y=8193), dict(F=0), dict(F=16385), dict(L=0), dict(L=1025),
                dict(dirs=None), dict(dirs=None, L=5), dict(dirs=None, F=1025, L=1025), dict(dirs=None, F=2000, L=1024)):
        assert call(**bad) == H.ERR_UNSUPPORTED, bad
    for bad in (dict(X=None), dict(Y=None), dict(ws=None), dict(w=None), dict(ks=None)):
        assert call(**bad) == H.ERR_ARG, bad
    assert not any(buf), "a refusal wrote"


# ---- 4. the refusals of the wrappers and of the model ---------------------------------------------------------------------------------
def test_every_operand_refusal_comes_before_a_launch():
    from multimodal_vae_comparison_amd import hipops as H, ops
    x, y = torch.randn(6, 3), torch.randn(5, 3)
    d = torch.from_numpy(R.draw(3, 4, 0))
    calls = H.CALLS[0]
    wide = torch.zeros(2, 1).expand(2, 1025)
    cases = [
        ("X is .*floating", (x.long(), y), {}), ("Y is .*floating", (x, y[0]), {}), ("X is ndarray", (x.numpy(), y), {}),
        ("X has 0 rows", (x[:0], y), {}), ("Y has 0 rows", (x, y[:0]), {}),
        ("X has 8193 rows", (torch.zeros(1, 3).expand(8193, 3), y), {}), ("Y has 8193 rows", (x, torch.zeros(1, 3).expand(8193, 3)), {}),
        ("X has F = 16385 features", (torch.zeros(2, 1).expand(2, 16385), torch.zeros(2, 1).expand(2, 16385)), {}),
        ("X has F = 0 features", (torch.zeros(2, 0), torch.zeros(2, 0)), {}),
        ("X has F = 3 features, Y F = 2", (x, y[:, :2]), {}),
        ("axis mode .*F = 1025", (wide, wide), {}),
        ("directions is .*float64", (x, y, d.float()), {}), ("directions is .*float64", (x, y, d[0]), {}),
        ("directions is list", (x, y, [[1.0, 0.0, 0.0]]), {}),
        (r"directions is \(4, 2\)", (x, y, d[:, :2].contiguous()), {}), (r"directions is \(0, 3\)", (x, y, d[:0]), {}),
        (r"directions is \(1025, 3\)", (x, y, torch.zeros(1025, 3, dtype=torch.float64)), {}),
        ("directions holds values that are not finite", (x, y, d * float("nan")), {}),
        ("X holds values that are not finite", (x * float("inf"), y), {}),
        ("Y holds values that are not finite", (x, torch.full((5, 3), float("nan"))), {}),
        ("X is on cpu; the kernel runs on the MI355X", (x, y, d), {}), ("X is on cpu", (x, y), {}),
        ("X is on cpu", (x, y, d.numpy()), {}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="swd_slices: .*" + match):
            ops.swd_slices(*args, **kwargs)
    for match, args, kwargs in [("n_directions = 0", (x, y), {"n_directions": 0}), ("n_directions = 1025", (x, y), {"n_directions": 1025}),
                                ("X and Y are floating", (x, None), {}), ("X has 0 rows", (x[:0], y), {}),
                                ("X has F = 16385", (torch.zeros(2, 1).expand(2, 16385),) * 2, {}),
                                ("X is on cpu", (x, y), {"n_directions": 3}), ("X is on cpu", (x, y), {"directions": d})]:
        with pytest.raises(ValueError, match="sliced_wasserstein: .*" + match):
            ops.sliced_wasserstein(*args, **kwargs)
    for match, args in [("axis mode", (wide, wide)), ("X is on cpu", (x, y)), ("Y is .*floating", (x, None)),
                        ("Y holds values that are not finite", (x, y * float("nan")))]:
        with pytest.raises(ValueError, match="marginal_tests: .*" + match):
            ops.marginal_tests(*args)
    assert H.CALLS[0] == calls, "a refusal came after a C call"


def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


def test_unimodal_vae_refuses_both_methods_by_name():
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    for name in ("latent_transport", "sliced_distances"):
        with pytest.raises(NotImplementedError) as e:
            getattr(vae, name)()
        assert "unimodal" in str(e.value) and f"TorchMMVAE.{name}" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="latent_transport needs eval mode"):
        model.latent_transport([cdsprites_batch(4, 6, seed=3)])
    with pytest.raises(RuntimeError, match="sliced_distances needs eval mode"):
        model.sliced_distances([cdsprites_batch(4, 6, seed=3)], {"mod_1": lambda x: x.flatten(1)})


def test_argument_errors_come_before_the_first_encoder_call(monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    calls = []
    monkeypatch.setattr(model, "_sample", lambda *a, **kw: calls.append(1))
    monkeypatch.setattr(model, "latents_for", lambda *a, **kw: calls.append(1))
    monkeypatch.setattr(model, "forward", lambda *a, **kw: calls.append(1))
    half = dict(batch, mod_2=dict(batch["mod_2"], data=None))
    one = dict(batch, mod_1=dict(batch["mod_1"], data=batch["mod_1"]["data"][:1]))
    big = dict(batch, mod_1=dict(batch["mod_1"], data=torch.zeros(1, 3, 64, 64).expand(8193, 3, 64, 64)))
    cases = [
        ("`batches` is empty", ([],), {}), ("n_directions = 0", ([batch],), {"n_directions": 0}),
        ("n_directions = 1025", ([batch],), {"n_directions": 1025}),
        ("must name modalities", ([batch],), {"given": [["mod_1"], ["mod_9"]]}),
        ("different conditioning subsets", ([batch],), {"given": [["mod_1"], ["mod_1"]]}),
        ("names a modality without data", ([half],), {}), ("1 rows of 8 latent dimensions", ([one],), {"given": [["mod_1"]]}),
        ("8193 rows of 8 latent dimensions", ([big],), {"given": [["mod_1"]]}),
        ("density is a result of fit_latent_density", ([batch],), {"density": {"mod_3": {}}}),
        (r"eps is \(4, 7\)", ([batch],), {"eps": torch.zeros(4, 7)}), ("eps is int", ([batch],), {"eps": 1}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="latent_transport: .*" + match):
            model.latent_transport(*args, **kwargs)
    flat = {"mod_1": lambda x: x.flatten(1)}
    cases = [
        ("`batches` is empty", ([], flat), {}), ("`features` maps modalities", ([batch], {"mod_9": len}), {}),
        ("a modality without data", ([half], flat), {}), ("n_directions = 0", ([batch], flat), {"n_directions": 0}),
        ("n_directions = 2000", ([batch], flat), {"n_directions": 2000}),
        ("8193 real rows", ([big], flat), {}), ("n_joint = 8193", ([batch], flat), {"n_joint": 8193}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="sliced_distances: .*" + match):
            model.sliced_distances(*args, **kwargs)
    assert not calls
    doc = type(model).latent_transport.__doc__
    assert "EVEN rows" in doc and "ODD rows" in doc and "independent" in doc
    assert "flatten(1)" in type(model).sliced_distances.__doc__ and "no classifier" in type(model).sliced_distances.__doc__


# ---- 5. the two model methods on scripted posteriors --------------------------------------------------------------------------------
def _scripted_ops(monkeypatch, seen, fail_at=None):
    """ops.sliced_wasserstein / ops.marginal_tests that record their operands and answer with sums of them"""
    from multimodal_vae_comparison_amd import ops

    def sliced(X, Y, n_directions=128, seed=0, directions=None):
        if fail_at is not None and len(seen) >= fail_at:
            raise ValueError("scripted failure")
        seen.append(("swd", X.clone(), Y.clone(), directions))
        v = X.double().sum() - Y.double().sum()
        return {"swd1": v, "swd2": v + 1, "max_sliced1": v + 2, "max_sliced2": v + 3}

    def marginal(X, Y):
        seen.append(("ks", X.clone(), Y.clone(), None))
        D = X.shape[1]
        return {"w1": torch.arange(D).double(), "w2": torch.ones(D).double(), "ks": torch.full((D,), 0.5).double(),
                "ks_p": np.full(D, 0.25), "ks_num": torch.ones(D).long(), "n_x": X.shape[0], "n_y": Y.shape[0]}
    monkeypatch.setattr(ops, "sliced_wasserstein", sliced)
    monkeypatch.setattr(ops, "marginal_tests", marginal)
    return ops


def test_latent_transport_on_scripted_posteriors(monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    names = list(model.vaes.keys())
    batches = [cdsprites_batch(4, 6, seed=3), cdsprites_batch(2, 6, seed=4)]
    N, D, asked = 6, 8, []

    def latents_for(batch, given, of=None):
        """row r of batch b under subset g: 100 (index of g) + 10 b + r in every dimension"""
        asked.append(tuple(given))
        b = 0 if len(batch[names[0]]["data"]) == 4 else 1
        rows = torch.arange(len(batch[names[0]]["data"])).float() + 10 * b + 100 * len(set(asked))
        return rows[:, None].expand(-1, D).clone()
    monkeypatch.setattr(model, "latents_for", latents_for)
    seen = []
    ops = _scripted_ops(monkeypatch, seen)
    eps = torch.randn(N, D, generator=torch.Generator().manual_seed(1))
    held = [e.clone() for e in (model._rng_state, model._eval_rng_state)]
    model.eps_override = marker = [torch.zeros(1)]
    res = model.latent_transport(batches, n_directions=5, seed=3, eps=eps)
    assert model.eps_override is marker and model._eval_draws is False
    assert torch.equal(model._rng_state, held[0]) and torch.equal(model._eval_rng_state, held[1]), "eps given: nothing is drawn"
    given = model.default_given()
    keys = ["+".join(g) for g in given]
    # all subsets' latents first, in the order of `given`, every batch of a subset in order
    assert asked == [tuple(g) for g in given for _ in batches]
    assert list(res) == ["prior", "pairs", "density", "n"] and res["n"] == N and res["density"] is None
    assert list(res["prior"]) == keys and list(res["pairs"]) == [f"{keys[a]}|{keys[b]}" for a, b in ((0, 1), (0, 2), (1, 2))]
    Z = [torch.cat([torch.arange(4.0), torch.arange(2.0) + 10]) + 100 * (i + 1) for i in range(3)]
    loc, scale = model.pz_params
    prior = (loc + scale * eps).contiguous()
    want = [(Z[i], None) for i in range(3)] + [(Z[a][0::2], Z[b][1::2]) for a, b in ((0, 1), (0, 2), (1, 2))]
    assert [s[0] for s in seen] == ["swd", "ks"] * 6
    for i, (zx, zy) in enumerate(want):
        for kind, X, Y, dirs in seen[2 * i:2 * i + 2]:
            assert torch.equal(X[:, 0], zx) and X.is_contiguous() and Y.is_contiguous()
            assert torch.equal(Y, prior) if zy is None else torch.equal(Y[:, 0], zy)
            if kind == "swd":      # one set of directions, the documented draw
                assert np.array_equal(dirs.numpy(), ops.swd_draw(D, 5, 3)) and dirs is seen[0][3]
    pair = res["pairs"][f"{keys[0]}|{keys[2]}"]
    assert (pair["n_x"], pair["n_y"]) == (3, 3) and set(pair) == {"swd1", "swd2", "max_sliced1", "max_sliced2", "w1", "w2",
                                                                  "ks", "ks_p", "n_x", "n_y"}
    v = float(Z[0][0::2].double().sum() * D - Z[2][1::2].double().sum() * D)
    assert (pair["swd1"], pair["swd2"], pair["max_sliced1"], pair["max_sliced2"]) == (v, v + 1, v + 2, v + 3)
    assert pair["w1"].tolist() == list(range(D)) and pair["ks_p"].tolist() == [0.25] * D and pair["ks"].dtype == torch.float64
    # the state comes back when the comparison raises, too
    seen.clear()
    _scripted_ops(monkeypatch, seen, fail_at=3)
    with pytest.raises(ValueError, match="scripted failure"):
        model.latent_transport(batches, eps=eps)
    assert model.eps_override is marker and model._eval_draws is False and torch.is_grad_enabled()
    assert torch.equal(model._rng_state, held[0]) and torch.equal(model._eval_rng_state, held[1])


def test_sliced_distances_on_scripted_generations(monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    names = list(model.vaes.keys())
    batches = [cdsprites_batch(4, 6, seed=3), cdsprites_batch(2, 6, seed=4)]
    shapes = {m: tuple(batches[0][m]["data"].shape[1:]) for m in names}
    calls = []

    def forward(batch):
        """generation k of the walk holds the value k + 1 everywhere, two rows more than the batch"""
        given = tuple(m for m in names if batch[m]["data"] is not None)
        B = max(len(batch[m]["data"]) for m in given)
        calls.append((given, B))
        loc = {m: torch.full((B + 2,) + shapes[m], float(len(calls))) for m in names}
        return types.SimpleNamespace(mods={m: types.SimpleNamespace(decoder_dist=types.SimpleNamespace(loc=loc[m])) for m in names})
    monkeypatch.setattr(model, "forward", forward)
    seen = []
    ops = _scripted_ops(monkeypatch, seen)
    flat = lambda x: x.flatten(1)[:, :7]
    held = [e.clone() for e in (model._rng_state, model._eval_rng_state)]
    model.eps_override = marker = [torch.zeros(1)]
    res = model.sliced_distances(batches, {names[0]: flat, names[1]: flat}, n_directions=4, seed=9)
    assert model.eps_override is marker and model._eval_draws is False
    assert torch.equal(model._rng_state, held[0]) and torch.equal(model._eval_rng_state, held[1])
    # per batch: the full batch, then one modality given at a time
    assert calls == [(tuple(names), 4), (names[:1] and (names[0],), 4), ((names[1],), 4), (tuple(names), 2), ((names[0],), 2),
                     ((names[1],), 2)]
    assert list(res) == names
    for i, m in enumerate(names):
        other = names[1 - i]
        assert list(res[m]) == ["recon", "cross", "joint", "n", "F"] and (res[m]["n"], res[m]["F"]) == (6, 7)
        assert list(res[m]["cross"]) == [other] and res[m]["joint"] is None
        mine = seen[2 * i:2 * i + 2]
        real = torch.cat([flat(b[m]["data"]).float() for b in batches])
        k = 2 if i == 0 else 1      # the cross-generation of m comes from the call with the OTHER modality given
        for (kind, X, Y, dirs), gen in zip(mine, ((0, 3), (k, k + 3))):
            assert kind == "swd" and torch.equal(X, real) and tuple(Y.shape) == (6, 7)
            assert Y[:4].eq(gen[0] + 1).all() and Y[4:].eq(gen[1] + 1).all()      # the first B rows of either batch's call
            assert dirs is seen[0][3] and np.array_equal(dirs.numpy(), ops.swd_draw(7, 4, 9))
        v = float(real.double().sum() - mine[0][2].double().sum())
        assert res[m]["recon"] == {"swd1": v, "swd2": v + 1, "max_sliced1": v + 2, "max_sliced2": v + 3, "n": 6}
    seen.clear()
    _scripted_ops(monkeypatch, seen, fail_at=1)
    with pytest.raises(ValueError, match="scripted failure"):
        model.sliced_distances(batches, {names[0]: flat})
    assert model.eps_override is marker and model._eval_draws is False and torch.is_grad_enabled()
    assert torch.equal(model._rng_state, held[0]) and torch.equal(model._eval_rng_state, held[1])


def test_trainer_wrappers_log_the_documented_names(monkeypatch):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods("mopoe", CD_MODS, 8, batch_size=4)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cpu")
    logged = []
    monkeypatch.setattr(tr, "log", lambda name, value, **kw: logged.append((name, float(value))))
    entry = {"swd1": 1.0, "swd2": 2.0, "max_sliced1": 3.0, "max_sliced2": 4.0, "n": 5}
    monkeypatch.setattr(tr.model, "sliced_distances", lambda *a, **k: {"mod_1": {
        "recon": entry, "cross": {"mod_2": dict(entry, swd2=2.5)}, "joint": dict(entry, swd2=2.75), "n": 5, "F": 3}})
    tr.sliced_distances([], {})
    assert logged == [("test_swd2_mod_1_recon", 2.0), ("test_swd2_mod_1_from_mod_2", 2.5), ("test_swd2_mod_1_joint", 2.75)]
    logged.clear()
    table = dict(entry, ks=torch.tensor([0.1, 0.7, 0.3], dtype=torch.float64))
    monkeypatch.setattr(tr.model, "latent_transport", lambda *a, **k: {"prior": {"mod_1": table, "mod_1+mod_2": table},
                                                                       "pairs": {}, "density": None, "n": 5})
    tr.latent_transport([])
    assert logged == [("test_swd2_prior_mod_1", 2.0), ("test_ks_max_prior_mod_1", 0.7),
                      ("test_swd2_prior_mod_1+mod_2", 2.0), ("test_ks_max_prior_mod_1+mod_2", 0.7)]
