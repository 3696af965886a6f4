"""GPU tests of the latent cluster analysis (csrc/cluster.hip), part by part: k-means, the statistics of
a partition, the silhouette, the limits and TorchMMVAE.cluster_latents end to end.  Everything is held to the float64
restatement with direct differences (tests/cluster_reference.py).  Labels, iteration counts and the best restart: exact
equality, after the test has asserted from the restatement alone that no row's two nearest centres were ever within 10^3
rounding bars of each other and that no cluster went empty.  Sums of distances: the bound of the Gram route carried through
the square root, which the restatement computes.  Nothing is held to the code under test."""
import numpy as np
import pytest
import torch

import cluster_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [f"{s[0]}x{s[1]}x{s[2]}" for s in R.SHAPES]
CASES = range(len(R.SHAPES))


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def host(t):
    return t.cpu().numpy()


def fair(F, ref, what):
    """the precondition of every exact comparison, from the restatement alone -> the rounding bar of a squared distance"""
    b = R.bar(F, ref["scale"])
    print(f"{what}: smallest gap between the two nearest centres {ref['gap']:.3e} = {ref['gap'] / b:.3g} bars (bar {b:.3e}); "
          f"n_iter {ref['n_iter'].tolist()}, converged {ref['converged'].tolist()}, best {ref['best']}")
    assert ref["gap"] >= 1e3 * b, "the inputs put a row too close to the border of two clusters: choose other inputs"
    assert not ref["ever_empty"], "a cluster went empty: choose other inputs"
    assert ref["best_margin"] >= 1e-9, "two different restarts are within 10^3 roundings of the best inertia: choose other inputs"
    return b


def same_fit(got, ref, X, what):
    """labels, n_iter, converged, best exact; centres within 4 F 2^-53 max|x| per element; inertia to 1e-12 relative"""
    F = X.shape[1]
    assert got["labels"].dtype == torch.int32 and got["centres"].dtype == torch.float64 and got["inertia"].dtype == torch.float64
    wrong = int((host(got["labels"]) != ref["labels"]).sum())
    err = float(np.abs(host(got["centres"]) - ref["centres"]).max())
    tol = 4.0 * F * R.U * float(np.abs(X).max())
    rel = float(np.abs(host(got["inertia"]) / ref["inertia"] - 1.0).max())
    print(f"{what}: {wrong} labels differ; centres off by {err:.3e} (allowed {tol:.3e}); inertia relative {rel:.3e}; "
          f"n_iter {host(got['n_iter']).tolist()}")
    assert wrong == 0
    assert host(got["n_iter"]).tolist() == ref["n_iter"].tolist() and host(got["converged"]).tolist() == ref["converged"].tolist()
    assert got["best"] == ref["best"] and host(got["empty"]).tolist() == ref["empty"].tolist()
    assert np.array_equal(host(got["counts"]), ref["counts"])
    assert err <= tol and rel <= 1e-12


def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


# ---- 1. k-means --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_kmeans(ops, i):
    X, init = R.case(i)
    ref = R.fit(i)
    fair(X.shape[1], ref, IDS[i])
    x = dev(X)
    got = ops.kmeans_fit(x, dev(init))
    same_fit(got, ref, X, IDS[i])
    assert same_bits(got, ops.kmeans_fit(x, dev(init))), "two runs differ"
    # both forms of init
    centres = dev(R.start_centres(X, init))
    assert same_bits(got, ops.kmeans_fit(x, centres)), "row numbers and the centres they name differ"
    # a restart alone gives the bits it gives beside the others
    for r in range(R.N_INIT):
        alone = ops.kmeans_fit(x, dev(init[r:r + 1]))
        for k in ("labels", "centres", "inertia", "n_iter", "converged", "empty", "counts"):
            assert torch.equal(alone[k][0], got[k][r]), (r, k)


@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_kmeans_stopped_at_three_iterations(ops, i):
    """the iteration limit: after the third update one more assignment, so that the labels are those of the centres"""
    X, init = R.case(i)
    ref = R.fit(i, 3)
    fair(X.shape[1], ref, IDS[i])
    got = ops.kmeans_fit(dev(X), dev(init), max_iter=3)
    same_fit(got, ref, X, IDS[i])
    nearest = R.sqdist_to(X.astype(np.float64), host(got["centres"])[0]).argmin(1)
    assert np.array_equal(host(got["labels"])[0], nearest)


def test_some_restart_is_stopped_by_the_limit():
    """(what makes the test above a test of the limit)"""
    assert any(not R.fit(i, 3)["converged"].all() for i in CASES) and all(R.fit(i)["converged"].all() for i in CASES)
    assert any(R.fit(i)["n_iter"].max() > 8 for i in CASES)      # more than one enqueued call of iterations


def test_an_empty_cluster_keeps_its_centre(ops):
    """restart 0: two equal start centres -- every tie goes to the lower index, the higher one has no rows at iteration 1 and
    must come back from that update unchanged (from then on it is a centre like any other: it lies on a row).  Restart 1:
    a start centre far from every row never has rows, counts at every update and never moves."""
    X, init = R.case(1)
    start = R.start_centres(X, init[:2]).copy()
    start[0, 2] = start[0, 0]
    start[1, 2] = 1e3
    tol = 4.0 * X.shape[1] * R.U * float(np.abs(X).max())
    for max_iter in (1, 300):
        ref = R.kmeans(X, start, max_iter)
        if max_iter == 1:
            assert ref["empty"].tolist() == [1, 1] and ref["gap"] == 0.0 and np.array_equal(ref["centres"][:, 2], start[:, 2])
        else:
            assert ref["converged"].all() and ref["empty"][0] >= 1 and ref["empty"][1] == ref["n_iter"][1] - 1 >= 2
            assert ref["counts"][1, 2] == 0
        got = ops.kmeans_fit(dev(X), dev(start), max_iter=max_iter)
        assert host(got["empty"]).tolist() == ref["empty"].tolist() and host(got["n_iter"]).tolist() == ref["n_iter"].tolist()
        assert host(got["converged"]).tolist() == ref["converged"].tolist()
        assert np.array_equal(host(got["labels"]), ref["labels"]) and np.array_equal(host(got["counts"]), ref["counts"])
        assert float(np.abs(host(got["centres"]) - ref["centres"]).max()) <= tol
        assert np.array_equal(host(got["centres"])[1, 2], start[1, 2]), "the centre of the empty cluster moved"
        if max_iter == 1:
            assert np.array_equal(host(got["centres"])[0, 2], start[0, 2]), "the centre of the empty cluster moved"


# ---- 2. statistics of a partition ----------------------------------------------------------------------------------------------------
def partitions():
    """(name, X, labels, C): the best k-means partition of every shape, and the crafted one"""
    out = [(IDS[i], R.case(i)[0], R.fit(i)["labels"][R.fit(i)["best"]], R.SHAPES[i][2]) for i in CASES]
    X, labels, _, _ = R.crafted()
    return out + [("crafted", X, labels, len(R.CRAFTED_SIZES))]


PARTS = range(len(R.SHAPES) + 1)
PART_IDS = IDS + ["crafted"]


@pytest.mark.parametrize("p", PARTS, ids=PART_IDS)
def test_cluster_stats(ops, p):
    what, X, labels, C = partitions()[p]
    ref = R.stats(X, labels, C)
    got = ops.cluster_stats(dev(X), dev(labels), C)
    assert np.array_equal(host(got["counts"]), ref["counts"])
    errs = {k: np.abs(host(got[k]) - ref[k]) for k in ("means", "within", "wdist")}
    tols = {"means": ref["tol_element"], "within": ref["tol_within"], "wdist": ref["tol_wdist"]}
    print(f"{what}: " + ", ".join(f"{k} uses {float((errs[k] / np.maximum(tols[k], 1e-300)).max()):.3g} of its bound" for k in errs))
    assert all(np.all(errs[k] <= tols[k]) for k in errs)
    ch, db = R.indices(ref)
    idx = ops.cluster_indices(got)
    assert abs(idx["calinski_harabasz"] / ch - 1.0) <= 1e-12 and abs(idx["davies_bouldin"] / db - 1.0) <= 1e-12
    again = ops.cluster_stats(dev(X), dev(labels), C)
    assert all(torch.equal(again[k], got[k]) for k in got), "two runs differ"


# ---- 3. silhouette -----------------------------------------------------------------------------------------------------------------
def check_silhouette(got, ref, labels, what):
    S, s = host(got["sums"]), host(got["samples"])
    assert got["sums"].dtype == torch.float64 and got["samples"].dtype == torch.float64 and isinstance(got["score"], float)
    assert np.array_equal(host(got["counts"]), ref["counts"])
    used = float((np.abs(S - ref["sums"]) / np.maximum(ref["tol_sums"], 1e-300)).max())
    assert np.all(np.abs(S - ref["sums"]) <= ref["tol_sums"]), f"{what}: sums off by {used:.3g} of the bound"
    # the final arithmetic, from the device's own sums
    mine = R.silhouette_from_sums(S, labels, ref["counts"])[0]
    assert float(np.abs(s - mine).max()) <= 4.0 * R.U, f"{what}: samples differ from those of the device's own sums"
    finite = np.isfinite(ref["tol_samples"])
    worst = float((np.abs(s - ref["samples"])[finite] / np.maximum(ref["tol_samples"][finite], 1e-300)).max())
    print(f"{what}: sums use {used:.3g} of their bound, samples {worst:.3g}; score {got['score']:.6f} ({ref['score']:.6f})")
    assert np.all(np.abs(s - ref["samples"])[finite] <= ref["tol_samples"][finite])
    assert np.all(s[ref["counts"][labels] == 1] == 0.0), "a member of a singleton cluster must score exactly 0"
    assert abs(got["score"] - ref["score"]) <= float(ref["tol_samples"][finite].mean()) + 4.0 * R.U


@pytest.mark.parametrize("p", PARTS, ids=PART_IDS)
def test_silhouette(ops, p):
    what, X, labels, C = partitions()[p]
    ref = R.silhouette(X, labels, C)
    x, lab = dev(X), dev(labels)
    got = ops.silhouette(x, lab, C)
    check_silhouette(got, ref, labels, what)
    again = ops.silhouette(x, lab, C)
    assert same_bits(got, again), "two runs differ"
    for chunks in (1, 2, 3, 1000):
        other = ops.silhouette(x, lab, C, chunks=chunks)
        check_silhouette(other, ref, labels, f"{what}, {chunks} chunk(s)")
        assert same_bits(other, ops.silhouette(x, lab, C, chunks=chunks)), "the same plan twice differs"


def test_the_shapes_cover_what_they_are_there_for(ops):
    """a singleton in the 16-cluster case; at N = 1100 clusters over several tiles and more than one chunk, and with one tile
    per chunk several chunks per cluster for the merge to add"""
    assert (R.fit(R.SINGLETON)["counts"][R.fit(R.SINGLETON)["best"]] == 1).any()
    counts = R.fit(5)["counts"][R.fit(5)["best"]]
    assert counts.min() > 64
    _, _, table, first = ops.silhouette_plan(counts, 1100, 0)
    assert len(table) > 1 and (table[:, 2] - table[:, 1]).max() > 1
    _, _, table, first = ops.silhouette_plan(counts, 1100, 1000)
    assert np.diff(first).min() > 1 and len(table) > len(counts)
    _, _, one_each, _ = ops.silhouette_plan(counts, 1100, 1)
    assert len(one_each) == len(counts)


def test_crafted_partition_in_detail(ops):
    """two singletons, two unused ids, a duplicated row: the ids without rows have a zero column and are ignored, the pair of
    equal rows is sqrt(rounding) apart at the most (left out by index, not by value)"""
    X, labels, _, (a, b) = R.crafted()
    ref = R.silhouette(X, labels, len(R.CRAFTED_SIZES))
    got = ops.silhouette(dev(X), dev(labels), len(R.CRAFTED_SIZES))
    S = host(got["sums"])
    assert np.all(S[:, [1, 5]] == 0.0) and host(got["counts"]).tolist() == list(R.CRAFTED_SIZES)
    singles = np.flatnonzero(np.isin(labels, (3, 6)))
    assert len(singles) == 2 and np.all(host(got["samples"])[singles] == 0.0) and np.all(S[singles, labels[singles]] == 0.0)
    # without the pair's own distance the two rows have the same sums: what is left of S[a, 0] - S[b, 0] is that distance twice
    assert labels[a] == labels[b] == 0 and ref["sums"][a, 0] == ref["sums"][b, 0]
    rest = R.distances(X)[a, (labels == 0) & (np.arange(len(X)) != b)].sum()
    assert abs(S[a, 0] - rest) <= ref["sqrt_bar"] + ref["tol_sums"][a, 0]
    # n_clusters None: the largest id + 1
    assert same_bits(got, ops.silhouette(dev(X), dev(labels)))


def test_all_rows_equal(ops):
    """the diagonal contributes nothing and a zero distance is no NaN: sums <= n_c sqrt(b)"""
    X = np.tile(R.case(1)[0][:1], (70, 1))
    labels = (np.arange(70) % 3).astype(np.int32)
    got = ops.silhouette(dev(X), dev(labels), 3)
    root = np.sqrt(R.bar(X.shape[1], float((X.astype(np.float64) ** 2).sum(1).max())))
    S = host(got["sums"])
    assert np.all(np.isfinite(S)) and np.all(S >= 0.0) and np.all(S <= host(got["counts"])[None, :] * root)
    assert np.all(np.isfinite(host(got["samples"]))) and np.isfinite(got["score"])


# ---- 4. limits --------------------------------------------------------------------------------------------------------------------------
def test_limits_raise_and_write_nothing(ops):
    from multimodal_vae_comparison_amd import hipops as H
    ones = torch.ones(70, 4, device=DEV)
    lab = torch.arange(70, device=DEV) % 3
    for bad in (torch.ones(4, 2049, device=DEV), torch.ones(16385, 2, device=DEV)):
        with pytest.raises(ValueError, match="MI355X path"):
            ops.kmeans_fit(bad, torch.tensor([[0, 1]], device=DEV))
        with pytest.raises(ValueError, match="MI355X path"):
            ops.silhouette(bad, torch.arange(len(bad), device=DEV) % 2)
        with pytest.raises(ValueError, match="MI355X path"):
            ops.cluster_stats(bad, torch.arange(len(bad), device=DEV) % 2, 2)
    with pytest.raises(ValueError, match="MI355X path"):
        ops.kmeans_fit(ones, torch.arange(65, device=DEV)[None, :])
    with pytest.raises(ValueError, match="MI355X path"):
        ops.kmeans_fit(ones, torch.arange(2, device=DEV)[None, :].repeat(65, 1))
    with pytest.raises(ValueError, match="MI355X path"):
        ops.kmeans_fit(ones, torch.tensor([[0, 1]], device=DEV), max_iter=1001)
    with pytest.raises(ValueError, match="MI355X path"):
        ops.kmeans_fit(ones[:3], torch.tensor([[0, 1, 2, 3]], device=DEV))
    with pytest.raises(ValueError, match="MI355X path"):
        ops.silhouette(torch.ones(70, 4, device=DEV), torch.arange(70, device=DEV))
    with pytest.raises(ValueError, match="two clusters with rows"):
        ops.silhouette(ones, torch.zeros(70, dtype=torch.int64, device=DEV), 3)
    with pytest.raises(ValueError, match="not finite"):
        ops.silhouette(torch.full((70, 4), float("nan"), device=DEV), lab)
    # the C entry points refuse the same shapes themselves and leave their outputs alone
    L, s, p, U = H.lib(), H.stream(), H.ptr, H.ERR_UNSUPPORTED
    x = torch.ones(64, 64, device=DEV)
    mu = torch.full((1 << 16,), -1.0, dtype=torch.float64, device=DEV)
    d2 = torch.full((20000,), -2.0, dtype=torch.float64, device=DEV)
    out = torch.full((1 << 16,), -3.0, dtype=torch.float64, device=DEV)
    li = torch.full((20000,), -4, dtype=torch.int32, device=DEV)
    ws = torch.full((1 << 16,), -5, dtype=torch.int32, device=DEV)
    for rows, F, C, R_ in ((4, 2049, 2, 1), (16385, 2, 2, 1), (0, 4, 2, 1), (4, 4, 65, 1), (4, 4, 0, 1), (4, 4, 2, 65), (4, 4, 2, 0)):
        assert L.mmvae_cluster_assign(p(x), p(mu), p(li), p(d2), rows, F, C, R_, 0, s) == U
        assert L.mmvae_cluster_means(p(x), p(li), p(mu), p(ws), rows, F, C, R_, s) == U
        assert L.mmvae_cluster_lloyd(p(x), p(mu), p(li), p(ws), rows, F, C, R_, 1, 1, 300, s) == U
        if F <= 2048:
            assert L.mmvae_cluster_spread(p(li), p(d2), p(ws), p(out), p(out), p(out), rows, C, R_, s) == U
    assert L.mmvae_cluster_assign(p(x), p(mu), p(li), p(d2), 4, 4, 2, 1, 2, s) == U
    for it0, n, most in ((1, 1, 1001), (0, 1, 300), (1, 0, 300), (300, 2, 300), (1, 1, 0)):
        assert L.mmvae_cluster_lloyd(p(x), p(mu), p(li), p(ws), 4, 4, 2, 1, it0, n, most, s) == U
    for rows, F, C, padded, chunks in ((4, 2049, 2, 128, 2), (16385, 2, 2, 128, 2), (0, 4, 2, 128, 2), (4, 4, 65, 128, 2),
                                      (4, 4, 2, 100, 2), (4, 4, 2, 0, 2), (4, 4, 2, 256, 2), (4, 4, 2, 128, 0), (4, 4, 2, 128, 3)):
        assert L.mmvae_cluster_sil_sums(p(x), p(d2), p(li), p(ws), p(ws), p(out), p(out), rows, F, C, padded, chunks, s) == U
    torch.cuda.synchronize()
    assert bool((mu == -1.0).all()) and bool((d2 == -2.0).all()) and bool((out == -3.0).all())
    assert bool((li == -4).all()) and bool((ws == -5).all())


# ---- 5. the metric end to end -----------------------------------------------------------------------------------------------------------
def _state(model):
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    drops = [m.state.clone() for m in model.modules() if isinstance(m, DropoutState)]
    grads = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    return model._rng_state.clone(), drops, grads


def _same_state(a, b):
    assert torch.equal(a[0], b[0]), "the training noise state moved"
    assert len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])), "a dropout counter moved"
    for x, y in zip(a[2], b[2]):
        assert (x is None and y is None) or torch.equal(x, y), "a gradient changed"


def _latent_case(mixing, seed):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    B, D = 6, 8
    torch.manual_seed(seed)
    cfg, dims = config_from_mods(mixing, CD_MODS, D, batch_size=B)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0")
    tr.model.eval()
    batches = [cdsprites_batch(B, 6, seed=s, device=DEV) for s in (3, 4)]
    g = torch.Generator().manual_seed(seed + 2)
    eps = [torch.randn(B, D, generator=g) for _ in range(64)]      # more than the latents_for calls draw
    return tr, batches, eps


@pytest.mark.parametrize("mixing", ["mopoe", "poe"])
def test_cluster_latents_end_to_end(hip_lib, mixing):
    from multimodal_vae_comparison_amd import ops
    B, C, n_init, seed = 6, 3, 3, 0      # (a draw after which no two restarts end within rounding of the best inertia)
    tr, batches, eps = _latent_case(mixing, 21)
    model = tr.model
    truth = (np.arange(2 * B) % 2).astype(np.int64)
    model.objective(batches[0])["loss"].backward()      # a gradient to watch
    torch.cuda.synchronize()
    before = _state(model)
    model.eps_override = [e.clone() for e in eps]
    out = tr.cluster_latents(batches, C, labels=truth, n_init=n_init, seed=seed)
    torch.cuda.synchronize()
    left = len(model.eps_override)
    model.eps_override = None
    _same_state(before, _state(model))
    assert model._eval_draws is False and torch.is_grad_enabled()
    given = model.default_given()
    assert list(out) == ["mod_1", "mod_2", "mod_1+mod_2"] == ["+".join(g) for g in given]

    # the latents rebuilt by hand, subset by subset in the same order of draws
    model.eps_override = [e.clone() for e in eps]
    zs = {"+".join(g): torch.cat([model.latents_for(b, g) for b in batches]).cpu().numpy() for g in given}
    assert len(model.eps_override) == left
    model.eps_override = None
    init = ops.kmeans_draw(2 * B, C, n_init, seed)
    assert np.array_equal(init, R.draw(2 * B, C, n_init, seed))
    logged = {}
    for key, Z in zs.items():
        assert Z.dtype == np.float32 and Z.shape == (2 * B, 8)
        ref = R.kmeans(Z, init)
        fair(8, ref, f"{mixing} {key}")
        r, best = out[key], ref["best"]
        assert np.array_equal(host(r["labels"]), ref["labels"][best]) and r["n_iter"] == ref["n_iter"][best]
        assert r["converged"] == bool(ref["converged"][best])
        assert host(r["restarts"]["n_iter"]).tolist() == ref["n_iter"].tolist()
        assert float(np.abs(host(r["centres"]) - ref["centres"][best]).max()) <= 4.0 * 8 * R.U * float(np.abs(Z).max())
        assert abs(r["inertia"] / ref["inertia"][best] - 1.0) <= 1e-12
        sil = R.silhouette(Z, ref["labels"][best], C)
        finite = np.isfinite(sil["tol_samples"])
        assert np.all(np.abs(host(r["silhouette_samples"]) - sil["samples"])[finite] <= sil["tol_samples"][finite])
        assert abs(r["silhouette"] - sil["score"]) <= float(sil["tol_samples"][finite].mean()) + 4.0 * R.U
        ch, db = R.indices(R.stats(Z, ref["labels"][best], C))
        assert abs(r["calinski_harabasz"] / ch - 1.0) <= 1e-12 and abs(r["davies_bouldin"] / db - 1.0) <= 1e-12
        agree = R.agreement(truth, ref["labels"][best])
        assert set(r["agreement"]) == {0} and all(abs(r["agreement"][0][n] - agree[n]) <= 1e-12 for n in R.AGREEMENT)
        own = R.silhouette(Z, truth, 2)
        assert set(r["label_silhouette"]) == {0}
        assert abs(r["label_silhouette"][0] - own["score"]) <= float(own["tol_samples"][np.isfinite(own["tol_samples"])].mean()) + 4.0 * R.U
        logged.update({f"test_cluster_silhouette_{key}": r["silhouette"], f"test_cluster_ch_{key}": r["calinski_harabasz"],
                       f"test_cluster_db_{key}": r["davies_bouldin"], f"test_cluster_ari_{key}_0": r["agreement"][0]["ari"],
                       f"test_cluster_nmi_{key}_0": r["agreement"][0]["nmi"],
                       f"test_cluster_purity_{key}_0": r["agreement"][0]["purity"],
                       f"test_cluster_label_silhouette_{key}_0": r["label_silhouette"][0]})
    assert {k: float(v) for k, v in tr.logged.items() if k.startswith("test_cluster_")} == logged
    _same_state(before, _state(model))
