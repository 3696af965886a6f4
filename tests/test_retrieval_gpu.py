"""GPU tests of the cross-modal retrieval of latents (csrc/retrieval.hip): the ranks, the ties, the
neighbour lists, the edges, the bit identity under column splits and beside other pairs, and TorchMMVAE.cross_modal_retrieval
end to end.  Everything is held to the float64 restatement by direct differences (tests/retrieval_reference.py) and to the
rounding bar derived there, 2 (D + 8) 2^-53 sum |terms| for a distance.  Counts and neighbour indices are compared EXACTLY:
before a case is compared, `fair` asserts from the restatement alone that every decision has a margin of 10^3 bars and that
the case tells something (many distinct ranks, fewer than half the rows at rank 1).  The tie cases are built from small
integers and powers of two, where every operation of both arithmetics is exact; the test asserts that too (the restatement
repeated in extended precision gives the same bits).  Nothing is held to the code under test."""
import numpy as np
import pytest
import torch

import retrieval_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEEP = 16
EXACT = [(N, D, m) for N, D in R.SHAPES for m in R.METRICS if not (m == "cosine" and D == 1)]


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def run(ops, loc, scale, metric, **kw):
    got = ops.retrieval_ranks(dev(loc), dev(scale) if metric in ("w2", "skl") else None, metric=metric, **kw)
    torch.cuda.synchronize()
    return got


def held(got, p, d, bar, match, keep, what):
    """pair p of a retrieval_ranks result against the restatement's distances: counts and indices exactly, distances within
    the bar -> the worst fraction of the bar"""
    dm, less, equal = R.ranks(d, match)
    nn_d, nn_idx = R.neighbours(d, keep)
    N = d.shape[0]
    for name, dtype, shape in (("d_match", torch.float64, (N,)), ("less", torch.int32, (N,)), ("equal", torch.int32, (N,)),
                               ("nn_d", torch.float64, (N, keep)), ("nn_idx", torch.int32, (N, keep))):
        assert got[name][p].dtype == dtype and tuple(got[name][p].shape) == shape, (what, name)
    g = {k: got[k][p].cpu().numpy() for k in ("d_match", "less", "equal", "nn_d", "nn_idx")}
    assert np.array_equal(g["less"], less), f"{what}: less differs in {int((g['less'] != less).sum())} rows"
    assert np.array_equal(g["equal"], equal), f"{what}: equal differs"
    assert np.array_equal(g["nn_idx"], nn_idx), f"{what}: nn_idx differs in {int((g['nn_idx'] != nn_idx).any(1).sum())} rows"
    def fraction(err, b):
        """the largest error as a fraction of its bar; a bar of 0 (an exact 0) admits an error of 0 and nothing else"""
        assert np.all(err[b == 0] == 0), f"{what}: an error where the bar is 0"
        return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0

    has = less >= 0
    m = np.where(has, np.arange(N) if match is None else match, 0)
    assert np.all(np.isnan(g["d_match"][~has]))
    worst = fraction(np.abs(g["d_match"][has] - dm[has]), bar[np.arange(N), m][has])
    filled = nn_idx >= 0
    assert np.all(np.isposinf(g["nn_d"][~filled]))
    rows = np.arange(N)[:, None].repeat(keep, 1)
    worst = max(worst, fraction(np.abs(g["nn_d"][filled] - nn_d[filled]), bar[rows[filled], nn_idx[filled]]))
    if keep > 1:
        assert np.all(g["nn_d"][:, 1:] >= g["nn_d"][:, :-1]), f"{what}: nn_d is not ascending"
    print(f"{what}: worst distance error {worst:.3g} of the bar; median rank "
          f"{np.median(1 + less[has] + equal[has]) if has.any() else float('nan')}")
    assert worst <= 1.0, (what, worst)
    return worst


# ---- 1. ranks and neighbours at the tile edges, every metric --------------------------------------------------------------------
@pytest.mark.parametrize("N,D,metric", EXACT)
def test_ranks_and_neighbours(ops, N, D, metric):
    c = R.case(N, D)
    got = run(ops, c["loc"], c["scale"], metric, match=dev(c["match"]), keep=KEEP)
    assert got["pairs"] == [(0, 1), (1, 0)]
    for p, (q, g) in enumerate(got["pairs"]):
        # (1, 0): the case's partners; (0, 1): the same list read as partners among the noisy rows -- strangers, any rank
        d, bar = R.pair_distances(metric, c["loc"][q], c["scale"][q], c["loc"][g], c["scale"][g])
        what = f"{N} x {D} {metric} {q}->{g}"
        margin = R.fair(d, bar, c["match"], KEEP, what)
        print(f"{what}: margin {margin:.3g} bars")
        held(got, p, d, bar, c["match"], KEEP, what)


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------------
def _exact_distances(metric, c):
    """the restatement of set 1 against set 0 of a tie case, and the assertion that its arithmetic was exact: repeated in
    extended precision it gives the same bits"""
    d, bar = R.pair_distances(metric, c["loc"][1], c["scale"][1], c["loc"][0], c["scale"][0])
    ql, qs, gl, gs = (a.astype(np.longdouble) for a in (c["loc"][1], c["scale"][1], c["loc"][0], c["scale"][0]))
    diff = ql[:, None, :] - gl[None, :, :]
    if metric == "l2":
        wide = (diff * diff).sum(-1)
    elif metric == "w2":
        wide = (diff * diff + (qs[:, None] - gs[None]) ** 2).sum(-1)
    elif metric == "skl":
        vq, vg = qs[:, None] ** 2, gs[None] ** 2
        wide = (((vq + diff * diff) / vg + (vg + diff * diff) / vq) / 2 - 1).sum(-1)
    else:      # D = 1: the sign of the product, or 1 beside a zero
        prod = ql[:, None, 0] * gl[None, :, 0]
        wide = np.where(prod == 0, 1, 1 - np.sign(prod))
    assert np.array_equal(d.astype(np.longdouble), wide), f"{metric}: the tie case is not exact"
    return d, bar


@pytest.mark.parametrize("metric", R.METRICS)
def test_ties_are_counted_and_ordered_by_index(ops, metric):
    c = R.tie_case(D=1) if metric == "cosine" else R.tie_case()
    N, dup = c["N"], c["dup"]
    d, bar = _exact_distances(metric, c)
    dm, less, equal = R.ranks(d)
    # from the restatement: the duplicated rows tie with their copies, the tie is exact, ranks are pessimistic
    assert np.all(equal[:2 * dup] >= 1) and equal[0] >= 2 and equal[N - 1] >= 2 and int((equal > 0).sum()) >= 2 * dup + 1
    nn_d, nn_idx = R.neighbours(d, 8)
    assert all(nn_idx[i, 0] == i and nn_idx[i, 1] == i + dup for i in range(1, dup)) or metric == "cosine"
    tied = nn_d[:, 1:] == nn_d[:, :-1]
    assert tied.any() and np.all(nn_idx[:, 1:][tied] > nn_idx[:, :-1][tied])
    got = run(ops, c["loc"], c["scale"], metric, pairs=[(1, 0)], keep=8)
    held(got, 0, d, bar, None, 8, f"ties {metric}")
    assert np.array_equal(got["d_match"][0].cpu().numpy(), dm) and np.array_equal(got["nn_d"][0].cpu().numpy(), nn_d)
    s = ops.retrieval_summary(got["less"][0], got["equal"][0], ks=(1,))
    want = R.summary(less, equal, (1,), N)
    assert s["tied_rows"] == want["tied_rows"] >= 2 * dup + 1 and s["recall@1"] == want["recall@1"] < 1.0
    rank = 1 + got["less"][0].cpu().numpy() + got["equal"][0].cpu().numpy()
    assert np.all(rank[:2 * dup] >= 2), "a tie counted as a hit"


@pytest.mark.parametrize("metric", R.METRICS)
def test_identical_rows_score_rank_n(ops, metric):
    N, D = 70, 3
    loc = np.broadcast_to(np.array([1.0, -2.0, 3.0], np.float32), (2, N, D)).copy()
    scale = np.full((2, N, D), 0.5, np.float32)
    got = run(ops, loc, scale, metric, keep=4)
    for p in range(2):
        assert got["less"][p].tolist() == [0] * N and got["equal"][p].tolist() == [N - 1] * N
        assert got["nn_idx"][p].tolist() == [[0, 1, 2, 3]] * N
        assert bool((got["nn_d"][p] == got["d_match"][p][:, None]).all()) and float(got["d_match"][p].abs().max()) <= 1e-15
    for s in ops.retrieval_summary(got["less"], got["equal"], ks=(1, 5, 10)):
        assert s["median_rank"] == N and s["recall@1"] == s["recall@5"] == s["recall@10"] == 0.0 and s["tied_rows"] == N
        assert s["normalised_rank"] == 1.0 and s["chance@10"] == 10 / N


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "skl"])
def test_rows_without_a_partner_and_partners_in_the_last_column(ops, metric):
    N, D = 65, 33      # (column 64 is the only column of the last staged tile, row 64 the only row of the last row tile)
    c = R.case(N, D)
    match = c["match"].copy()
    match[::7] = -1
    match[[3, 10, 64]] = N - 1
    d, bar = R.pair_distances(metric, c["loc"][1], c["scale"][1], c["loc"][0], c["scale"][0])
    R.fair(d, bar, match, KEEP, f"edges {metric}")
    got = run(ops, c["loc"], c["scale"], metric, pairs=[(1, 0)], match=match, keep=KEEP)
    held(got, 0, d, bar, match, KEEP, f"edges {metric}")
    none = match < 0
    assert got["less"][0].cpu().numpy()[none].tolist() == [-1] * int(none.sum()) == got["equal"][0].cpu().numpy()[none].tolist()
    assert bool((got["nn_idx"][0][torch.from_numpy(none).to(DEV)] >= 0).all()), "a row without a partner still has neighbours"
    s = ops.retrieval_summary(got["less"][0], got["equal"][0], ks=(1,), n_gallery=N)
    assert s["n"] == int((~none).sum())


@pytest.mark.parametrize("keep", [0, 1, 16])
def test_keep(ops, keep):
    c = R.case(64, 8)
    for metric in ("cosine", "w2"):
        r = R.reference(64, 8, metric)
        R.fair(r["d"], r["bar"], c["match"], KEEP, f"keep {keep} {metric}")
        got = run(ops, c["loc"], c["scale"], metric, pairs=[(1, 0)], match=dev(c["match"]), keep=keep)
        assert tuple(got["nn_d"].shape) == tuple(got["nn_idx"].shape) == (1, 64, keep)
        held(got, 0, r["d"], r["bar"], c["match"], keep, f"keep {keep} {metric}")


def test_keep_beyond_the_rows_pads(ops):
    rs = np.random.RandomState(9)
    loc = rs.standard_normal((2, 5, 3)).astype(np.float32)
    scale = rs.uniform(0.1, 1, (2, 5, 3)).astype(np.float32)
    for metric in R.METRICS:
        d, bar = R.pair_distances(metric, loc[0], scale[0], loc[1], scale[1])
        R.fair(d, bar, None, KEEP, f"pad {metric}")      # (the gaps; 5 rows: ranks 1 .. 5)
        got = run(ops, loc, scale, metric, pairs=[(0, 1)], keep=KEEP)
        held(got, 0, d, bar, None, KEEP, f"pad {metric}")
        assert got["nn_idx"][0][:, 5:].tolist() == [[-1] * 11] * 5 and bool(torch.isinf(got["nn_d"][0][:, 5:]).all())


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------------------------
OUT = ("d_match", "less", "equal", "nn_d", "nn_idx")


def same_bits(a, b, pa=None, pb=None):
    return all(torch.equal(a[k] if pa is None else a[k][pa], b[k] if pb is None else b[k][pb]) for k in OUT)


@pytest.mark.parametrize("metric", R.METRICS)
def test_column_splits_and_runs_give_the_same_bits(ops, metric):
    from multimodal_vae_comparison_amd import hipops
    N, D = 600, 8
    assert hipops.lib().mmvae_retrieval_chunks(N, 2) == 3      # (the default plan splits the 19 staged tiles)
    c = R.case(N, D)
    base = run(ops, c["loc"], c["scale"], metric, match=dev(c["match"]), keep=KEEP)
    for chunks in (0, 1, 3, 5, 19, 1000):
        again = run(ops, c["loc"], c["scale"], metric, match=dev(c["match"]), keep=KEEP, chunks=chunks)
        assert same_bits(base, again), f"{metric}: chunks = {chunks} changes the bits"
    r = R.reference(N, D, metric)
    R.fair(r["d"], r["bar"], c["match"], KEEP, f"splits {metric}")
    held(base, 1, r["d"], r["bar"], c["match"], KEEP, f"splits {metric}")


@pytest.mark.parametrize("metric", R.METRICS)
def test_a_pair_alone_and_beside_others(ops, metric):
    N, D, S = 65, 33, 3
    c = R.case(N, D, S=S)
    every = run(ops, c["loc"], c["scale"], metric, match=dev(c["match"]), keep=KEEP)
    assert every["pairs"] == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    for p, pair in enumerate(every["pairs"]):
        alone = run(ops, c["loc"], c["scale"], metric, pairs=[pair], match=dev(c["match"]), keep=KEEP, chunks=2)
        assert same_bits(every, alone, p, 0), f"{metric}: pair {pair} alone differs from the same pair beside five others"
    q, g = every["pairs"][4]
    d, bar = R.pair_distances(metric, c["loc"][q], c["scale"][q], c["loc"][g], c["scale"][g])
    R.fair(d, bar, c["match"], KEEP, f"six pairs {metric}")
    held(every, 4, d, bar, c["match"], KEEP, f"six pairs {metric}")


def test_sixteen_sets_in_one_launch(ops):
    N, D, S = 65, 8, 16
    c = R.case(N, D, S=S)
    every = run(ops, c["loc"], c["scale"], "w2", keep=4)
    assert len(every["pairs"]) == 240 and every["pairs"] == ops.retrieval_pairs(S)
    for p in (0, 7, 121, 239):
        q, g = every["pairs"][p]
        alone = run(ops, c["loc"], c["scale"], "w2", pairs=[(q, g)], keep=4)
        assert same_bits(every, alone, p, 0), f"pair {(q, g)} of 240"
        d, bar = R.pair_distances("w2", c["loc"][q], c["scale"][q], c["loc"][g], c["scale"][g])
        R.fair(d, bar, None, 4, f"240 pairs, pair {p}")
        held(every, p, d, bar, None, 4, f"240 pairs, pair {p}")


# ---- 5. the metric end to end ------------------------------------------------------------------------------------------------------------
def _snapshot(model):
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    return [model._rng_state] + [m.state for m in model.modules() if isinstance(m, DropoutState)]


def _build(mixing, prior="normal", D=8, sizes=(5, 5, 5)):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    torch.manual_seed(51)
    mods = [dict(m, private=4) for m in CD_MODS] if mixing == "dmvae" else CD_MODS
    cfg, dims = config_from_mods(mixing, mods, D, batch_size=sizes[0], prior=prior)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    return model, [cdsprites_batch(B, 6, seed=3 + i, device=DEV) for i, B in enumerate(sizes)]


FIELDS = {"recall@1", "recall@5", "chance@1", "chance@5", "median_rank", "mean_rank", "mrr", "normalised_rank", "tied_rows", "n"}


def _check_pairs(ops, out, keys, loc, scale, metric, keep, labels, what):
    """the result of cross_modal_retrieval against ops.retrieval_ranks on the same sets (bit for bit) and against the
    restatement on them"""
    N = loc.shape[1]
    again = ops.retrieval_ranks(loc, scale, metric=metric, keep=keep)
    ln, sn = loc.cpu().numpy(), None if scale is None else scale.cpu().numpy()
    assert list(out) == [f"{keys[a]}->{keys[b]}" for a, b in again["pairs"]] + ["mean"]
    for p, (a, b) in enumerate(again["pairs"]):
        r = out[f"{keys[a]}->{keys[b]}"]
        assert set(r) == FIELDS | {"d_match", "rank", "nn_idx"} | ({"label_precision"} if labels is not None else set())
        assert torch.equal(r["d_match"], again["d_match"][p]) and torch.equal(r["nn_idx"], again["nn_idx"][p])
        assert r["rank"].dtype == torch.int32 and torch.equal(r["rank"], (1 + again["less"][p] + again["equal"][p]).cpu())
        d, bar = R.pair_distances(metric, ln[a], None if sn is None else sn[a], ln[b], None if sn is None else sn[b])
        dm, less, equal = R.ranks(d)
        # (the model's own posteriors: the gaps are asserted, what the ranks look like is the model's affair)
        rank = 1 + less + equal
        print(f"{what} {keys[a]}->{keys[b]}: ranks {sorted(rank.tolist())}")
        held(again, p, d, bar, None, keep, f"{what} {keys[a]}->{keys[b]}")
        want = R.summary(less, equal, (1, 5), N)
        assert all(abs(r[k] - want[k]) <= 1e-15 for k in want), (r, want)
        if labels is not None:
            _, nn_idx = R.neighbours(d, keep)
            for col in range(labels.shape[1]):
                lp = R.label_precision(nn_idx, labels[:, col], labels[:, col], (1, 5))
                got_lp = r["label_precision"][col]
                assert set(got_lp) == {1, 5} and all(abs(got_lp[k][n] - lp[k][n]) <= 1e-15 for k in lp for n in ("precision", "hit"))
    n_pairs = len(again["pairs"])
    assert set(out["mean"]) == FIELDS
    assert out["mean"]["mrr"] == pytest.approx(sum(out[k]["mrr"] for k in out if k != "mean") / n_pairs, abs=1e-15)
    return again


def _gaps(ops, loc, scale, metric, keep, what):
    """the precondition of the exact comparison on sets that come from a model: the gaps of `fair`, from the restatement"""
    ln, sn = loc.cpu().numpy(), None if scale is None else scale.cpu().numpy()
    for a, b in ops.retrieval_pairs(loc.shape[0]):
        d, bar = R.pair_distances(metric, ln[a], None if sn is None else sn[a], ln[b], None if sn is None else sn[b])
        Nq = d.shape[0]
        for i in range(Nq):
            order = np.lexsort((np.arange(Nq), d[i]))
            dd, bb = d[i, order], bar[i, order]
            assert float(((dd[1:] - dd[:-1]) / np.maximum(bb[1:], bb[:-1])).min()) >= R.MARGIN, f"{what}: a gap below the margin"


@pytest.mark.parametrize("mixing", ["poe", "moe", "mopoe", "dmvae"])
def test_cross_modal_retrieval_end_to_end(ops, mixing):
    model, batches = _build(mixing)
    names, D, N, keep = list(model.vaes.keys()), model.n_latents, 15, 10
    labels = torch.stack([torch.arange(N) % 2, torch.arange(N) % 3], 1)
    mine = model.eps_override = [torch.zeros(5, D)]
    before = [t.clone() for t in _snapshot(model)]
    ev = model._eval_rng_state.clone()

    # the posteriors are deterministic: disentanglement returns the same loc and scale for the same batches
    dis = model.disentanglement(batches)
    loc = torch.stack([dis[m]["loc"] for m in names]).contiguous()
    scale = torch.stack([dis[m]["scale"] for m in names]).contiguous()
    assert loc.shape == (2, N, D) and not torch.equal(loc[0], loc[1])
    for metric in R.METRICS:
        out = model.cross_modal_retrieval(batches, metric=metric, ks=(1, 5), keep=keep, labels=labels)
        torch.cuda.synchronize()
        _gaps(ops, loc, scale if metric in ("w2", "skl") else None, metric, keep, f"{mixing} {metric}")
        _check_pairs(ops, out, names, loc, scale if metric in ("w2", "skl") else None, metric, keep, labels.numpy(),
                     f"{mixing} posterior {metric}")
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model))), "the noise state or a dropout counter moved"
    assert model.eps_override is mine and len(mine) == 1 and model._eval_draws is False and torch.is_grad_enabled()
    model.eps_override = None

    # use="sample": the sets are latents_for's; with recorded draws they are forward()'s, bit for bit
    shapes, orig = [], model._draw

    def rec(b, d, dv):
        shapes.append((b, d))
        return orig(b, d, dv)
    model._draw = rec
    try:
        plain = model.cross_modal_retrieval(batches, use="sample", ks=(1, 5), keep=keep)
    finally:
        del model._draw
    assert not torch.equal(model._eval_rng_state, ev), "without recorded draws the evaluation generator draws"
    assert list(plain) == [f"{names[0]}->{names[1]}", f"{names[1]}->{names[0]}", "mean"] and shapes
    g = torch.Generator().manual_seed(57)
    eps = [torch.randn(1, b, d, generator=g) for b, d in shapes]
    for metric in ("l2", "cosine"):
        model.eps_override = [e.clone() for e in eps]
        out = model.cross_modal_retrieval(batches, metric=metric, use="sample", ks=(1, 5), keep=keep)
        assert model.eps_override == [], "the recorded draws are consumed as forward() consumes them"
        model.eps_override = [e.clone() for e in eps]
        z = torch.stack([torch.cat([model.latents_for(b, [m]) for b in batches]).float() for m in names]).contiguous()
        model.eps_override = None
        assert z.shape == (2, N, D)
        _gaps(ops, z, None, metric, keep, f"{mixing} sample {metric}")
        _check_pairs(ops, out, names, z, None, metric, keep, None, f"{mixing} sample {metric}")
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model))), "the noise state or a dropout counter moved"

    # a conditioning subset of two modalities is a set like any other
    both = model.cross_modal_retrieval(batches, use="sample", given=[[names[0]], names], ks=(1,), keep=1)
    assert list(both) == [f"{names[0]}->{'+'.join(names)}", f"{'+'.join(names)}->{names[0]}", "mean"]

    model.train()
    with pytest.raises(RuntimeError, match="cross_modal_retrieval needs eval mode"):
        model.cross_modal_retrieval(batches)
    model.eval()
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model)))


def test_laplace_posteriors_refuse_the_gaussian_distances_by_name(ops):
    model, batches = _build("moe", prior="laplace")
    names = list(model.vaes.keys())
    for metric in ("skl", "w2"):
        with pytest.raises(NotImplementedError, match=f"cross_modal_retrieval: metric '{metric}' .*Laplace"):
            model.cross_modal_retrieval(batches, metric=metric)
    out = model.cross_modal_retrieval(batches, metric="l2", ks=(1, 5), keep=4)
    dis = model.disentanglement(batches)
    loc = torch.stack([dis[m]["loc"] for m in names]).contiguous()
    _gaps(ops, loc, None, "l2", 4, "laplace moe l2")
    _check_pairs(ops, out, names, loc, None, "l2", 4, None, "laplace moe l2")
    assert model._eval_draws is False and model.eps_override is None
