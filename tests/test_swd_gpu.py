"""GPU tests of the sliced Wasserstein distances and marginal KS tests (csrc/swd.hip): `w` of every
shape of tests/swd_reference.py within the bounds derived there of the numpy longdouble restatement and `ks` equal to it, with
drawn directions and in axis mode; two runs to the bit; guard values around every buffer; exact ties (-0.0 among +0.0,
duplicated rows); a direction alone, first and last of sixteen; the formulas of ops.sliced_wasserstein and ops.marginal_tests;
TorchMMVAE.latent_transport and sliced_distances against the ops called by hand.  No graph is captured here."""
import numpy as np
import pytest
import torch

import swd_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def run(ops, c):
    return ops.swd_slices(dev(c.X), dev(c.Y), dev(c.dirs))


def guarded(ops, c):
    """the C entry point on buffers of the caller's, each between two guard blocks -> (w, ks) as ops.swd_slices shapes them"""
    H, G, mark = ops.H, 512, 12345.678
    x, y, d = dev(c.X), dev(c.Y), dev(c.dirs)
    need = H.lib().mmvae_swd_ws_doubles(c.n_x, c.n_y, c.F, c.L)
    assert need == c.L * (c.n_x + c.n_y)
    sizes = {"ws": need, "w": 2 * c.L, "ks": c.L}
    buf = {k: torch.full((G + v + G,), mark, dtype=torch.float64, device=DEV) for k, v in sizes.items()}
    at = {k: b.data_ptr() + 8 * G for k, b in buf.items()}
    H.call("mmvae_swd_slices", H.ptr(x), H.ptr(y), None if d is None else H.ptr(d), at["ws"], at["w"], at["ks"], c.n_x, c.n_y,
           c.F, c.L, H.stream())
    torch.cuda.synchronize()
    for k, b in buf.items():
        assert bool((b[:G] == mark).all()) and bool((b[G + sizes[k]:] == mark).all()), f"a guard of {k} was written"
    return buf["w"][G:G + 2 * c.L].view(c.L, 2).clone(), buf["ks"][G:G + c.L].view(torch.int64).clone()


def check(ops, c, what):
    """held to the restatement; two runs and the guarded call to the bit -> (w, ks)"""
    assert c.gap_ok, (what, "two pooled projections are nearly tied")
    w, ks = run(ops, c)
    assert w.dtype == torch.float64 and tuple(w.shape) == (c.L, 2) and ks.dtype == torch.int64 and tuple(ks.shape) == (c.L,)
    f1, f2 = c.held(w.cpu().numpy(), ks.cpu().numpy())
    gap = float((c.gaps / np.maximum(c.e, 1e-300)).min())
    print(f"{what}: W_1 at {f1:.3g}, W_2^2 at {f2:.3g} of their bounds; ks equal (largest D = "
          f"{int(ks.max()) / (c.n_x * c.n_y):.4g}); smallest pooled gap {gap:.3g} projection bounds")
    again = run(ops, c)
    assert torch.equal(again[0], w) and torch.equal(again[1], ks), "two runs differ"
    gw, gk = guarded(ops, c)
    assert torch.equal(gw, w) and torch.equal(gk, ks)
    return w, ks


# ---- 1. every shape, with drawn directions and in axis mode ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_drawn_directions(ops, shape):
    check(ops, R.case(*shape), f"{shape} drawn")


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[2] <= 1024], ids=lambda s: "x".join(map(str, s)))
def test_axis_mode(ops, shape):
    c = R.case(*shape, axis=True)
    assert c.L == c.F and not c.e.any()
    check(ops, c, f"{shape} axis")


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------------
def test_ties_in_axis_mode(ops):
    """integer values in {-2 .. 2}, -0.0 among +0.0: the projection is exact, w is held to the summation term alone"""
    c = R.ties_case(True)
    assert not c.e.any() and np.any(np.signbit(c.X) & (c.X == 0)) and np.any(~np.signbit(c.X) & (c.X == 0))
    w, ks = check(ops, c, "ties, axis")
    assert w[5].tolist() == [0.0, 0.0] and int(ks[5]) == 0, "a constant column"
    # the signs of the zeros do not matter: all of them +0.0 gives the same bits
    plain = ops.swd_slices(dev(c.X) + 0.0, dev(c.Y) + 0.0)
    assert not np.any(np.signbit((c.X + np.float32(0.0))[c.X == 0]))
    assert torch.equal(plain[0], w) and torch.equal(plain[1], ks)
    same = ops.swd_slices(dev(c.X), dev(c.X))
    assert torch.count_nonzero(same[0]) == 0 and torch.count_nonzero(same[1]) == 0
    flipped = ops.swd_slices(dev(c.X), dev(c.X[::-1]))
    assert torch.count_nonzero(flipped[0]) == 0 and torch.count_nonzero(flipped[1]) == 0


def test_ties_with_drawn_directions(ops):
    """a row twice more in X and twice in Y: the five copies project to the same bits, whichever set they sit in"""
    c = R.ties_case(False)
    assert np.array_equal(c.X[3], c.X[11]) and np.array_equal(c.X[3], c.Y[7])
    check(ops, c, "ties, drawn")
    # X against itself in another order, through the projections: zeros, exactly
    same = ops.swd_slices(dev(c.X), dev(c.X[::-1]), dev(c.dirs))
    assert torch.count_nonzero(same[0]) == 0 and torch.count_nonzero(same[1]) == 0


# ---- 3. bit identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 63, 8, 16), (257, 130, 33, 16), (1000, 1024, 5, 32)], ids=lambda s: "x".join(map(str, s)))
def test_a_direction_alone_first_and_last_of_sixteen(ops, shape):
    c = R.case(*shape)
    x, y = dev(c.X), dev(c.Y)
    w, ks = ops.swd_slices(x, y, dev(c.dirs))
    for l in (0, 7, c.L - 1):
        alone = ops.swd_slices(x, y, dev(c.dirs[l:l + 1]))
        assert torch.equal(alone[0][0], w[l]) and torch.equal(alone[1][0], ks[l]), f"direction {l} alone differs"
        for place in (0, 15):
            others = np.array(R.draw(c.F, 16, 77))
            others[place] = c.dirs[l]
            moved = ops.swd_slices(x, y, dev(others))
            assert torch.equal(moved[0][place], w[l]) and torch.equal(moved[1][place], ks[l]), (l, place)
    # more rows of either set leave the projections of the others as they are: the head of X against Y, as a subset
    head = ops.swd_slices(x[:40].contiguous(), y, dev(c.dirs))
    ref = R.Case(np.array(c.X[:40]), np.array(c.Y), np.array(c.dirs))
    ref.held(head[0].cpu().numpy(), head[1].cpu().numpy())


def test_axis_mode_on_a_column_is_the_column_alone(ops):
    c = R.case(257, 130, 33, 16, axis=True)
    w, ks = run(ops, c)
    for d in (0, 16, 32):
        col = ops.swd_slices(dev(c.X[:, d:d + 1]), dev(c.Y[:, d:d + 1]))
        assert torch.equal(col[0][0], w[d]) and torch.equal(col[1][0], ks[d])


# ---- 4. the formulas on top ----------------------------------------------------------------------------------------------------------
def test_by_hand(ops):
    """X = {0, 1}, Y = {0, 1, 2} on one axis: W_1 = 1 / 2, W_2^2 = 1 / 2, ks = 2 of 6"""
    x, y = torch.tensor([[0.0], [1.0]], device=DEV), torch.tensor([[0.0], [1.0], [2.0]], device=DEV)
    w, ks = ops.swd_slices(x, y)
    assert w.tolist() == [[0.5, 0.5]] and ks.tolist() == [2]
    t = ops.marginal_tests(x, y)
    assert t["ks"].tolist() == [2 / 6] and t["ks_num"].tolist() == [2] and (t["n_x"], t["n_y"]) == (2, 3)
    assert t["w1"].tolist() == [0.5] and t["w2"].tolist() == [0.5 ** 0.5] and t["ks_p"].tolist() == [ops.ks_p_value(1 / 3, 2, 3)]
    w, ks = ops.swd_slices(y, x, torch.tensor([[-2.0]], dtype=torch.float64, device=DEV))      # (directions are used as given)
    assert w.tolist() == [[1.0, 2.0]] and ks.tolist() == [2]


def test_sliced_wasserstein_and_marginal_tests_are_the_formulas(ops):
    c = R.case(300, 211, 256, 8)
    x, y = dev(c.X), dev(c.Y)
    out = ops.sliced_wasserstein(x, y, n_directions=8, seed=0)
    assert list(out) == ["swd1", "swd2", "max_sliced1", "max_sliced2", "w", "ks", "directions"]
    assert np.array_equal(out["directions"].cpu().numpy(), c.dirs) and out["directions"].dtype == torch.float64
    w, ks = ops.swd_slices(x, y, dev(c.dirs))
    assert torch.equal(out["w"], w) and torch.equal(out["ks"], ks)
    assert torch.equal(out["swd1"], w[:, 0].mean()) and torch.equal(out["swd2"], w[:, 1].mean().sqrt())
    assert torch.equal(out["max_sliced1"], w[:, 0].max()) and torch.equal(out["max_sliced2"], w[:, 1].max().sqrt())
    ref = c.ref["w"].astype(np.float64)
    assert abs(float(out["swd1"]) - ref[:, 0].mean()) <= c.b1.max() + 1e-15 * ref[:, 0].mean()
    assert abs(float(out["swd2"]) ** 2 - ref[:, 1].mean()) <= c.b2.max() + 1e-15 * ref[:, 1].mean()
    given = ops.sliced_wasserstein(x, y, directions=c.dirs)      # (a host array goes to the rows' device)
    assert torch.equal(given["w"], w) and float(out["max_sliced1"]) >= float(out["swd1"]) > 0
    a = R.case(300, 211, 256, 8, axis=True)
    t = ops.marginal_tests(x, y)
    aw, aks = ops.swd_slices(x, y)
    assert list(t) == ["w1", "w2", "ks", "ks_p", "ks_num", "n_x", "n_y"] and (t["n_x"], t["n_y"]) == (300, 211)
    assert torch.equal(t["w1"], aw[:, 0]) and torch.equal(t["w2"], aw[:, 1].sqrt()) and torch.equal(t["ks_num"], aks)
    assert np.array_equal(t["ks"].cpu().numpy(), a.ref["ks"] / (300 * 211)) and np.array_equal(aks.cpu().numpy(), a.ref["ks"])
    assert np.array_equal(t["ks_p"], ops.ks_p_value(a.ref["ks"] / (300 * 211), 300, 211)) and t["ks_p"].shape == (256,)
    # Y is 0.7 N(0, 1) + 0.3 against N(0, 1): most dimensions are told apart, and the same law is not
    assert np.mean(t["ks_p"] < 0.01) > 0.9
    half = ops.marginal_tests(x[0::2].contiguous(), x[1::2].contiguous())
    assert np.mean(half["ks_p"] < 0.01) < 0.05


def test_refusals_on_the_device(ops):
    x, y = torch.randn(6, 3, device=DEV), torch.randn(5, 3, device=DEV)
    calls = ops.H.CALLS[0]
    with pytest.raises(ValueError, match="X holds values that are not finite"):
        ops.swd_slices(x * float("nan"), y)
    with pytest.raises(ValueError, match="X is on cuda:0, Y on cpu"):
        ops.swd_slices(x, y.cpu())
    with pytest.raises(ValueError, match=r"directions is \(2, 4\)"):
        ops.swd_slices(x, y, torch.zeros(2, 4, dtype=torch.float64, device=DEV))
    assert ops.H.CALLS[0] == calls


# ---- 5. the metrics end to end -------------------------------------------------------------------------------------------------------
def _snapshot(model):
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    return [t.clone() for t in [model._rng_state] + [m.state for m in model.modules() if isinstance(m, DropoutState)]]


def _restore(model, saved):
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    for t, s in zip([model._rng_state] + [m.state for m in model.modules() if isinstance(m, DropoutState)], saved):
        t.copy_(s)


def _build(mixing, data, D=8, sizes=(6, 4)):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, MS_MODS, cdsprites_batch, config_from_mods, mnist_svhn_batch
    torch.manual_seed(67)
    cfg, dims = config_from_mods(mixing, CD_MODS if data == "cdsprites" else MS_MODS, D, batch_size=sizes[0])
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0")
    tr.model.eval()
    batches = [cdsprites_batch(B, 6, seed=7 + i, device=DEV) if data == "cdsprites" else mnist_svhn_batch(B, seed=7 + i, device=DEV)
               for i, B in enumerate(sizes)]
    return tr, batches


def _train_forward(model, batch):
    model.train()
    with torch.no_grad():
        out = model.forward(batch)
    model.eval()
    return [out.mods[m].decoder_dist.loc.clone() for m in model.vaes]


SCALARS = ("swd1", "swd2", "max_sliced1", "max_sliced2")


@pytest.mark.parametrize("mixing,data", [("mopoe", "cdsprites"), ("poe", "cdsprites"), ("moe", "mnist_svhn")])
def test_latent_transport_and_sliced_distances(ops, mixing, data):
    tr, batches = _build(mixing, data)
    model = tr.model
    names, N, D, L, seed = list(model.vaes.keys()), 10, 8, 16, 5
    given = model.default_given()
    keys = ["+".join(g) for g in given]
    before, ev = _snapshot(model), model._eval_rng_state.clone()
    first = _train_forward(model, batches[0])      # the training-mode forward() that the calls below must leave as it is
    _restore(model, before)
    grads = [p.grad for p in model.parameters()]
    eps = torch.randn(N, D, generator=torch.Generator().manual_seed(3))

    # ---- latent_transport: the keys and the draw order of latent_two_sample, the ops by hand
    res = tr.latent_transport(batches, n_directions=L, seed=seed, eps=eps)
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model))), "the noise state or a dropout counter moved"
    assert all(a is b for a, b in zip(grads, (p.grad for p in model.parameters()))) and torch.is_grad_enabled()
    assert model.eps_override is None and model._eval_draws is False
    pairs = [f"{keys[a]}|{keys[b]}" for a in range(len(keys)) for b in range(a + 1, len(keys))]
    assert list(res) == ["prior", "pairs", "density", "n"] and res["n"] == N and res["density"] is None
    assert list(res["prior"]) == keys and list(res["pairs"]) == pairs
    after = model._eval_rng_state.clone()
    model._eval_rng_state.copy_(ev)
    two = model.latent_two_sample(batches, permutations=3, seed=seed, eps=eps)
    assert list(two["prior"]) == keys and list(two["pairs"]) == pairs and two["n"] == N
    assert torch.equal(model._eval_rng_state, after), "latent_transport and latent_two_sample draw differently"
    model._eval_rng_state.copy_(ev)
    Z = [torch.cat([model.latents_for(b, g) for b in batches]).float().contiguous() for g in given]
    loc, scale = model.pz_params
    prior = (loc + scale * eps.to(DEV)).contiguous()
    dirs = ops.swd_draw(D, L, seed)

    def same(entry, X, Y):
        s, t = ops.sliced_wasserstein(X, Y, directions=dirs), ops.marginal_tests(X, Y)
        assert set(entry) == set(SCALARS) | {"w1", "w2", "ks", "ks_p", "n_x", "n_y"}
        assert all(entry[k] == float(s[k]) for k in SCALARS) and entry["swd2"] > 0
        assert all(torch.equal(entry[k], t[k].cpu()) and tuple(entry[k].shape) == (D,) for k in ("w1", "w2", "ks"))
        assert np.array_equal(entry["ks_p"].numpy(), t["ks_p"]) and (entry["n_x"], entry["n_y"]) == (X.shape[0], Y.shape[0])

    for k, z in zip(keys, Z):
        same(res["prior"][k], z, prior)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            same(res["pairs"][f"{keys[a]}|{keys[b]}"], Z[a][0::2].contiguous(), Z[b][1::2].contiguous())
    logged = {k: float(v) for k, v in tr.logged.items() if k.startswith(("test_swd2_prior_", "test_ks_max_prior_"))}
    want = {f"test_swd2_prior_{k}": res["prior"][k]["swd2"] for k in keys}
    want.update({f"test_ks_max_prior_{k}": float(res["prior"][k]["ks"].max()) for k in keys})
    assert logged == want

    # ---- sliced_distances on the raw pixels: the sets of _walk_generations, rebuilt by hand from the same generator state
    # (the captions of a CdSprites+ batch are shorter than the decoder's prior generations: pixels of the image alone there)
    mods = names if data == "mnist_svhn" else names[:1]
    flat = {m: (lambda x: x.flatten(1)) for m in mods}
    NJ = 5
    model._eval_rng_state.copy_(ev)
    out = tr.sliced_distances(batches, flat, n_directions=L, seed=seed, n_joint=NJ)
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model)))
    assert model.eps_override is None and model._eval_draws is False and torch.is_grad_enabled()
    model._eval_rng_state.copy_(ev)
    sets = {}
    with model._eval_noise():
        for batch in batches:
            B = len(batch[names[0]]["data"])
            full = model.forward(batch)
            for m in mods:
                sets.setdefault((m, "recon"), []).append(full.mods[m].decoder_dist.loc.flatten(1)[:B].float().clone())
            for g in names:
                if any(m != g for m in mods):
                    cross = model.forward(model._given_only(batch, [g]))
                    for m in mods:
                        if m != g:
                            sets.setdefault((m, g), []).append(cross.mods[m].decoder_dist.loc.flatten(1)[:B].float().clone())
        z = model._prior_sample(NJ, None, "by hand")
        for m in mods:
            sets[(m, "joint")] = [model.vaes[m].dec({"latents": z, "masks": None})[0].flatten(1).float()]
    assert list(out) == mods
    drawn = {}
    for m in mods:
        real = torch.cat([b[m]["data"].flatten(1).float() for b in batches])
        F = real.shape[1]
        drawn.setdefault(F, ops.swd_draw(F, L, seed))
        r = out[m]
        assert list(r) == ["recon", "cross", "joint", "n", "F"] and (r["n"], r["F"]) == (N, F)
        assert list(r["cross"]) == [g for g in names if g != m]
        for tag, entry, key in [("recon", r["recon"], (m, "recon")), ("joint", r["joint"], (m, "joint"))] + \
                [(f"from_{g}", r["cross"][g], (m, g)) for g in r["cross"]]:
            rows = torch.cat(sets[key])
            s = ops.sliced_wasserstein(real, rows, directions=drawn[F])
            assert entry == dict({k: float(s[k]) for k in SCALARS}, n=rows.shape[0]), (m, tag)
            assert entry["n"] == (NJ if tag == "joint" else N) and entry["max_sliced2"] >= entry["swd2"] > 0
            assert float(tr.logged[f"test_swd2_{m}_{tag}"]) == entry["swd2"]
            print(f"{mixing} {m} {tag}: F = {F}, swd2 {entry['swd2']:.6g}, max-sliced {entry['max_sliced2']:.6g}")

    # ---- the next training-mode forward() is the one it would have been
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model)))
    second = _train_forward(model, batches[0])
    assert all(torch.equal(a, b) for a, b in zip(first, second)), "the next training forward() changed"
