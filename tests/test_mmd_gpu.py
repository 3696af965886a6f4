"""GPU tests of the kernel two-sample test (csrc/mmd.hip): every entry of `sums` and `row_sums` of
every case of tests/mmd_reference.py against the numpy longdouble restatement, within 16 x the error of the float64
restatement (at least 1e-13 of the entry's sum of |k_ij|); the chunk plans; p-values to equality; bit identity of a
relabelling alone, in a batch and at another position; guard values around every buffer; TorchMMVAE.latent_two_sample
against ops.mmd_two_sample called by hand.  No graph is captured here."""
import ctypes

import numpy as np
import pytest
import torch

import mmd_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def run(ops, c, chunks=0, member="case"):
    """ops.mmd_sums with the restatement's own parameters (the automatic width has a test of its own)"""
    member = c.member if isinstance(member, str) else member
    return ops.mmd_sums(dev(c.X), dev(c.Y), None if member is None else dev(member), kernel=c.kernel, params=c.params,
                        chunks=chunks)


def held(c, sums, row_sums, what, rows=None):
    """every entry within its bound of the longdouble restatement -> the largest errors, in bounds.  `rows`: the rows of
    the restatement's sums that `sums` holds (default: all)"""
    ref = c.ld["sums"] if rows is None else c.ld["sums"][rows]
    bound = c.bound["sums"] if rows is None else c.bound["sums"][rows]
    assert sums.dtype == torch.float64 and tuple(sums.shape) == ref.shape
    assert row_sums.dtype == torch.float64 and tuple(row_sums.shape) == (c.n,)
    es = np.abs(sums.cpu().numpy().astype(R.LD) - ref).astype(np.float64)
    er = np.abs(row_sums.cpu().numpy().astype(R.LD) - c.ld["row_sums"]).astype(np.float64)
    rel = es / np.maximum(c.ld["abs_sums"].astype(np.float64) if rows is None else c.ld["abs_sums"][rows].astype(np.float64),
                          1e-300)
    print(f"{what}: sums {np.max(es / bound):.3g} bounds (largest error {rel.max():.3g} of sum |k|; the float64 restatement "
          f"{np.max(c.err['sums'] / np.maximum(c.ld['abs_sums'].astype(np.float64), 1e-300)):.3g}), row sums "
          f"{np.max(er / c.bound['row_sums']):.3g} bounds")
    assert np.all(np.isfinite(sums.cpu().numpy())) and np.all(np.isfinite(row_sums.cpu().numpy()))
    assert np.all(es <= bound), (what, np.max(es / bound))
    assert np.all(er <= c.bound["row_sums"]), (what, np.max(er / c.bound["row_sums"]))


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_sums(ops, name):
    c = R.case(name)
    sums, row_sums, params = run(ops, c)
    held(c, sums, row_sums, f"{name}, {ops.H.lib().mmvae_mmd_chunks(c.n)} chunk(s)")
    assert params == c.params
    again = run(ops, c)
    assert torch.equal(again[0], sums) and torch.equal(again[1], row_sums), "two runs differ"


@pytest.mark.parametrize("name", list(R.PLANS))
def test_chunk_plans(ops, name):
    """two plans regroup fp64 sums: each is held to the restatement, not to another plan; each is reproducible"""
    c = R.case(name)
    most = (c.n + 63) // 64
    assert R.PLANS[name][-1] == most and ops.H.lib().mmvae_mmd_chunks(c.n) <= most
    for chunks in R.PLANS[name] + (most + 3,):      # (more chunks than column tiles: one per tile)
        sums, row_sums, _ = run(ops, c, chunks=chunks)
        held(c, sums, row_sums, f"{name}, chunks = {chunks}")
        again = run(ops, c, chunks=chunks)
        assert torch.equal(again[0], sums) and torch.equal(again[1], row_sums), f"two runs with {chunks} chunks differ"
    assert torch.equal(run(ops, c, chunks=most + 3)[0], run(ops, c, chunks=most)[0])


def test_automatic_width(ops):
    """params None: gamma_s = 1 / (scale_s m2), c_s = scale_s m2 with m2 the mean of d^2 over the pooled pairs"""
    for name in ("n300-D8", "offset-imq", "n129-D1-S8"):
        c = R.case(name)
        sums, row_sums, params = ops.mmd_sums(dev(c.X), dev(c.Y), dev(c.member), kernel=c.kernel, scales=c.scales)
        assert len(params) == len(c.params)
        # the closed form in float64, two routes: within a few roundings of the D x n terms (offset: a variance of rows
        # near 1000 keeps nine digits on either route)
        assert np.allclose(params, c.params, rtol=1e-8 if name.startswith("offset") else 1e-12, atol=0.0), (params, c.params)
        again = ops.mmd_sums(dev(c.X), dev(c.Y), dev(c.member), kernel=c.kernel, params=params)
        assert torch.equal(again[0], sums) and torch.equal(again[1], row_sums)
    c = R.case("dup-energy")
    assert ops.mmd_sums(dev(c.X), dev(c.Y), kernel="energy")[2] == ()


def test_identical_rows_give_zero_not_nan(ops):
    """d = 0 exactly between rows with equal bits, far from the origin too: the energy kernel's root sees 0, never a
    negative rounding"""
    row = (np.random.RandomState(3).randn(1, 33) * 100 + 1000).astype(np.float32)
    X, Y = np.repeat(row, 70, 0), np.repeat(row, 5, 0)
    sums, row_sums, _ = ops.mmd_sums(dev(X), dev(Y), dev(R.draw(70, 5, 3, 0)), kernel="energy")
    assert torch.count_nonzero(sums) == 0 and torch.count_nonzero(row_sums) == 0
    sums, row_sums, _ = ops.mmd_sums(dev(X), dev(Y), dev(R.draw(70, 5, 3, 0)), kernel="rbf", params=(0.5, 3.0))
    assert sums[:, 0].tolist() == [70.0 * 69] * 4 and sums[:, 1].tolist() == [20.0] * 4 and sums[:, 2].tolist() == [350.0] * 4
    assert row_sums.tolist() == [74.0] * 75
    c = R.case("dup-energy")
    K = c.ld["K"]
    assert np.sum(K == 0) == c.n + 90      # (the diagonal and the ninety pairs of the ten copies)


# ---- 2. p-values: integer counts, compared exactly ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.NAMES if R.CASES[n][4] > 0])
def test_p_values(ops, name):
    c = R.case(name)
    assert c.apart() > 1.0      # (the host test holds this on the reference: no count can turn on a rounding)
    out = ops.mmd_two_sample(dev(c.X), dev(c.Y), member=dev(c.member), kernel=c.kernel, params=c.params)
    est = np.concatenate([[float(out["mmd2"])], out["null"].cpu().numpy()])
    e = np.abs(est.astype(R.LD) - c.mmd2).astype(np.float64)
    # the three quotients and two additions of the estimate: a few roundings of the terms' magnitudes beside the sums' bounds
    assert np.all(e <= 2.0 * c.mmd2_bound), (name, np.max(e / c.mmd2_bound))
    print(f"{name}: p = {out['p_value']} (restatement {c.p_value}), mmd2 = {float(out['mmd2']):.6g}")
    assert out["p_value"] == c.p_value
    drawn = ops.mmd_two_sample(dev(c.X), dev(c.Y), permutations=c.P, seed=c.draw_seed, kernel=c.kernel, params=c.params)
    assert np.array_equal(drawn["member"].cpu().numpy(), c.member) and drawn["p_value"] == c.p_value
    assert torch.equal(drawn["sums"], out["sums"])
    null = out["null"].cpu().numpy()
    assert abs(float(out["null_mean"]) - null.mean()) <= 1e-12 * np.abs(null).max()
    assert abs(float(out["null_std"]) - null.std()) <= 1e-12 * np.abs(null).max()
    if name == "same":
        assert out["p_value"] > 0.05
    if name == "shifted":
        assert out["p_value"] == 1.0 / (1 + c.P) and float(out["z"]) > 10.0


def test_no_relabelling(ops):
    c = R.case("n191-D16-P0-imq")
    out = ops.mmd_two_sample(dev(c.X), dev(c.Y), permutations=0, kernel=c.kernel, params=c.params)
    assert out["p_value"] == 1.0 and tuple(out["null"].shape) == (0,) and tuple(out["sums"].shape) == (1, 3)
    assert abs(float(out["mmd2"]) - float(c.mmd2[0])) <= 2.0 * c.mmd2_bound[0]


# ---- 3. bit identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n300-D8", "n257-D40-imq-S8", "65x128-D33-Pblock-energy"])
def test_a_relabelling_alone_in_a_batch_and_elsewhere(ops, name):
    """row 1 + p does not depend on P, on the other relabellings or on its place in `member` (nor on which block of
    columns holds it: the cases with more than one block put p on both sides of the border)"""
    c = R.case(name)
    sums, row_sums, _ = run(ops, c)
    back = run(ops, c, member=c.member[::-1])
    assert torch.equal(back[0][1:].flip(0), sums[1:]) and torch.equal(back[0][0], sums[0]) and torch.equal(back[1], row_sums)
    for p in sorted({0, c.P // 2, c.P - 1, min(c.P - 1, R.PBLOCK - R.EXTRA - 1), min(c.P - 1, R.PBLOCK - R.EXTRA)}):
        alone = run(ops, c, member=c.member[p:p + 1])
        assert torch.equal(alone[0][1], sums[1 + p]), f"relabelling {p} alone differs from itself in the batch"
        assert torch.equal(alone[0][0], sums[0]) and torch.equal(alone[1], row_sums)
    none = run(ops, c, member=None)
    assert torch.equal(none[0][0], sums[0]) and torch.equal(none[1], row_sums)
    # the observed split handed in as a relabelling is the observed split
    first = run(ops, c, member=R.splits(c.n_x, c.n_y, None))
    assert torch.equal(first[0][1], first[0][0])


@pytest.mark.parametrize("name", ["2x2", "n129-D1-S8", "n257-D40-imq-S8", "n191-D16-P0-imq"])
def test_guard_values_stay(ops, name):
    """the C entry point on buffers of the caller's, each between two guard blocks"""
    c = R.case(name)
    H, G, mark = ops.H, 512, 12345.678
    x, y, member = dev(c.X), dev(c.Y), dev(c.member)
    need = H.lib().mmvae_mmd_ws_doubles(c.n, c.D, c.P, 0)
    sizes = {"ws": need, "sums": 3 * (1 + c.P), "row_sums": c.n}
    buf = {k: torch.full((G + v + G,), mark, dtype=torch.float64, device=DEV) for k, v in sizes.items()}
    at = {k: b.data_ptr() + 8 * G for k, b in buf.items()}
    host = (ctypes.c_double * max(len(c.params), 1))(*c.params)
    H.call("mmvae_mmd_sums", H.ptr(x), H.ptr(y), H.ptr(member) if c.P else None, at["ws"], at["sums"], at["row_sums"], c.n_x,
           c.n_y, c.D, c.P, H.MMD_KERNELS[c.kernel], ctypes.addressof(host), len(c.params), 0, H.stream())
    torch.cuda.synchronize()
    for k, b in buf.items():
        assert bool((b[:G] == mark).all()) and bool((b[G + sizes[k]:] == mark).all()), f"a guard of {k} was written"
    sums, row_sums, _ = run(ops, c)
    assert torch.equal(buf["sums"][G:G + sizes["sums"]].view(1 + c.P, 3), sums)
    assert torch.equal(buf["row_sums"][G:G + c.n], row_sums)


def test_refusals_on_the_device(ops):
    c = R.case("n129-D1-S8")
    x, y = dev(c.X), dev(c.Y)
    with pytest.raises(ValueError, match="X has 1 rows"):
        ops.mmd_sums(x[:1], y)
    with pytest.raises(ValueError, match="Y has 1 rows"):
        ops.mmd_sums(x, y[:1])
    bad = np.array(c.member)
    bad[2, np.flatnonzero(bad[2] == 0)[0]] = 1
    with pytest.raises(ValueError, match="every relabelling keeps"):
        ops.mmd_sums(x, y, dev(bad))
    bad = np.array(c.member)
    bad[1, np.flatnonzero(bad[1] == 1)[:2]] = (2, 0)
    with pytest.raises(ValueError, match="values from 0 to 2"):
        ops.mmd_sums(x, y, dev(bad))
    with pytest.raises(ValueError, match="is on cpu"):
        ops.mmd_sums(x, y, torch.from_numpy(np.array(c.member)))
    calls = ops.H.CALLS[0]
    with pytest.raises(ValueError):
        ops.mmd_sums(x, y, dev(c.member[:, :-1]))
    assert ops.H.CALLS[0] == calls


# ---- 4. the metric end to end --------------------------------------------------------------------------------------------------------
def _snapshot(model):
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    return [t.clone() for t in [model._rng_state] + [m.state for m in model.modules() if isinstance(m, DropoutState)]]


def _build(mixing, D=8, sizes=(32, 32)):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    torch.manual_seed(61)
    mods = [dict(m, private=4) for m in CD_MODS] if mixing == "dmvae" else CD_MODS
    cfg, dims = config_from_mods(mixing, mods, D, batch_size=sizes[0])
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    return model, [cdsprites_batch(B, 6, seed=7 + i, device=DEV) for i, B in enumerate(sizes)]


FIELDS = ("mmd2", "p_value", "null_mean", "null_std", "z")


@pytest.mark.parametrize("mixing", ["mopoe", "moe", "mmvm", "dmvae"])
def test_latent_two_sample(ops, mixing):
    model, batches = _build(mixing)
    names, N, P, seed = list(model.vaes.keys()), 64, 50, 5
    given = model.default_given()
    keys = ["+".join(g) for g in given]
    before, ev = _snapshot(model), model._eval_rng_state.clone()
    grads = [p.grad for p in model.parameters()]
    res = model.latent_two_sample(batches, permutations=P, seed=seed)
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model))), "the noise state or a dropout counter moved"
    assert all(a is b for a, b in zip(grads, (p.grad for p in model.parameters()))) and torch.is_grad_enabled()
    assert model.eps_override is None and model._eval_draws is False
    assert not torch.equal(model._eval_rng_state, ev), "the evaluation generator draws"
    assert list(res) == ["prior", "pairs", "density", "n"] and res["n"] == N and res["density"] is None
    assert list(res["prior"]) == keys == [names[0], names[1], "+".join(names)]
    assert list(res["pairs"]) == [f"{keys[0]}|{keys[1]}", f"{keys[0]}|{keys[2]}", f"{keys[1]}|{keys[2]}"]

    # by hand, from the same state of the evaluation generator: the latents of every subset first, then the prior draws
    model._eval_rng_state.copy_(ev)
    Z = [torch.cat([model.latents_for(b, g) for b in batches]).float().contiguous() for g in given]
    with model._eval_noise():
        priors = [model._prior_sample(N, None, "by hand")[0] for _ in given]
    assert all(tuple(z.shape) == (N, 8) for z in Z + priors)

    def same(entry, X, Y):
        out = ops.mmd_two_sample(X, Y, permutations=P, seed=seed)
        assert set(entry) == set(FIELDS) | {"params", "n_x", "n_y"}
        for k in FIELDS:
            assert entry[k] == float(out[k]), k
        assert entry["params"] == out["params"] and (entry["n_x"], entry["n_y"]) == (X.shape[0], Y.shape[0])
        assert 1.0 / (1 + P) <= entry["p_value"] <= 1.0

    for k, z, p in zip(keys, Z, priors):
        same(res["prior"][k], z, p)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        same(res["pairs"][f"{keys[a]}|{keys[b]}"], Z[a][0::2].contiguous(), Z[b][1::2].contiguous())

    # recorded prior draws; another kernel; one subset pair only
    eps = torch.randn(N, 8, generator=torch.Generator().manual_seed(3))
    model._eval_rng_state.copy_(ev)
    got = model.latent_two_sample(batches, given=[[names[1]], names], kernel="energy", permutations=P, seed=seed, eps=eps)
    loc, scale = model.pz_params
    prior = (loc + scale * eps.to(DEV)).contiguous()
    model._eval_rng_state.copy_(ev)
    Z2 = [torch.cat([model.latents_for(b, g) for b in batches]).float().contiguous() for g in ([names[1]], names)]
    out = ops.mmd_two_sample(Z2[0], prior, permutations=P, seed=seed, kernel="energy")
    assert got["prior"][names[1]]["mmd2"] == float(out["mmd2"]) and got["prior"][names[1]]["params"] == ()
    assert list(got["pairs"]) == [f"{names[1]}|{'+'.join(names)}"]
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model)))


def test_latent_two_sample_against_a_fitted_density(ops):
    model, batches = _build("mopoe")
    names = list(model.vaes.keys())
    density = model.fit_latent_density(batches, 2, given=[names], n_init=2, max_iter=20)
    ev = model._eval_rng_state.clone()
    res = model.latent_two_sample(batches, given=[[names[0]], names], permutations=20, seed=2, density=density)
    key = "+".join(names)
    assert list(res["density"]) == [key]
    model._eval_rng_state.copy_(ev)
    Z = [torch.cat([model.latents_for(b, g) for b in batches]).float().contiguous() for g in ([names[0]], names)]
    with model._eval_noise():
        for _ in range(2):
            model._prior_sample(64, None, "by hand")
    drawn = model.sample_latent_density(density[key], 64, seed=2)["latents"]
    out = ops.mmd_two_sample(Z[1], drawn, permutations=20, seed=2)
    assert res["density"][key]["mmd2"] == float(out["mmd2"]) and res["density"][key]["p_value"] == out["p_value"]
