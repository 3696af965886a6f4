"""GPU tests of precision, recall, density and coverage (csrc/manifold.hip), part by part: the squared
norms, the radii, the cross pass, manifold_prdc, the limits and TorchMMVAE.manifold_metrics end to end.  Everything is held
to the float64 restatement with direct differences (tests/manifold_reference.py).  Distances: the rounding bound of the
Gram route, 8 F 2^-53 max_i |x_i|^2.  Counts and the four scalars: exact equality, after the test has asserted from the
restatement alone that no compared distance lies within 10^3 such bounds of its radius.  Nothing is held to the code under
test."""
import numpy as np
import pytest
import torch

import digit_reference as DR
import manifold_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [f"{s[0]}x{s[1]}x{s[2]}k{s[3]}" for s in R.SHAPES]


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def fair(F, ref, what):
    """the precondition of every exact comparison, from the restatement alone -> the rounding bar"""
    b = R.bar(F, ref["scale"])
    print(f"{what}: smallest |d^2 - rad^2| = {ref['margin']:.3e} = {ref['margin'] / b:.3g} bars (bar {b:.3e}); "
          + ", ".join(f"{n} {ref[n]:.6g}" for n in R.SCALARS))
    assert ref["margin"] >= 1e3 * b, "the inputs put a distance too close to a radius: choose other inputs"
    return b


# ---- 1. squared norms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=IDS)
def test_sqnorms(ops, i):
    Rr, G, _, ref = R.case(i)
    b = R.bar(Rr.shape[1], ref["scale"])
    for X in (Rr, G):
        got = ops.manifold_sqnorms(dev(X))
        err = float(np.abs(got.cpu().numpy() - R.sqnorms(X)).max())
        print(f"{X.shape}: |x|^2 error {err:.3e} = {err / b:.3g} bars")
        assert got.dtype == torch.float64 and err <= b
        assert torch.equal(ops.manifold_sqnorms(dev(X)), got)


# ---- 2. radii -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=IDS)
def test_radii(ops, i):
    Rr, G, k, ref = R.case(i)
    b = R.bar(Rr.shape[1], ref["scale"])
    for X, want in ((Rr, ref["rad2_real"]), (G, ref["rad2_fake"])):
        x = dev(X)
        got = ops.manifold_radii(x, k)
        err = float(np.abs(got.cpu().numpy() - want).max())
        plan = ops.H.lib().mmvae_manifold_chunks(len(X), len(X))
        print(f"{X.shape} k={k}, {plan} chunk(s): rad^2 error {err:.3e} = {err / b:.3g} bars")
        assert got.dtype == torch.float64 and got.shape == (len(X),) and err <= b
        assert torch.equal(ops.manifold_radii(x, k), got), "two runs differ"
        for chunks in (1, 2, 3, 1000):
            assert torch.equal(ops.manifold_radii(x, k, chunks=chunks), got), f"the plan with {chunks} chunks differs"


def test_more_neighbours_than_one_list_holds_of_a_chunk(ops):
    """every k up to 16 (the limit) on 40 rows in one tile: an epilogue thread meets ten columns at the most, so from k = 10
    on the k-th neighbour comes out of the merge of a row's four lists alone; all three list sizes (4, 8, 16 slots)"""
    X = R.features(40, 7, 1)
    D = R.sqdist(X, X)
    b = R.bar(7, float(R.sqnorms(X).max()))
    for k in range(1, 17):
        err = float(np.abs(ops.manifold_radii(dev(X), k).cpu().numpy() - R.radii(X, k, D)).max())
        assert err <= b, (k, err, b)


def test_a_duplicated_row_is_a_neighbour_at_zero(ops):
    """three equal rows: left out by index, not by distance -- the other two are neighbours at 0 (within the rounding of
    |x|^2 + |x|^2 - 2 x . x: the norms are summed in feature order, the product on the MFMA)"""
    X = np.array(R.case(1)[0])
    X[40] = X[3]
    X[69] = X[3]
    b = R.bar(X.shape[1], float(R.sqnorms(X).max()))
    D = R.sqdist(X, X)
    for k in (1, 2, 3):
        want, got = R.radii(X, k, D), ops.manifold_radii(dev(X), k).cpu().numpy()
        assert np.all(want[[3, 40, 69]] == 0.0) == (k < 3) and np.all(want[np.setdiff1d(np.arange(len(X)), (3, 40, 69))] > 1e6 * b)
        assert np.abs(got - want).max() <= b and np.all(got >= 0.0), k


# ---- 3. the cross pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=IDS)
def test_cross(ops, i):
    Rr, G, k, ref = R.case(i)
    b = fair(Rr.shape[1], ref, IDS[i])
    r, g = dev(Rr), dev(G)
    # (queries, manifold, the restatement's radii of the manifold, the expected counts, the expected nearest d^2)
    D = R.sqdist(G, Rr)
    for what, q, a, rad, hits, near in (("generated in real spheres", g, r, ref["rad2_real"], ref["hit_real"], D.min(1)),
                                        ("real in generated spheres", r, g, ref["rad2_fake"], ref["hit_fake"], ref["near_real"])):
        count, mind2 = ops.manifold_cross(q, a, dev(rad))
        err = float(np.abs(mind2.cpu().numpy() - near).max())
        wrong = int((count.cpu().numpy() != hits).sum())
        print(f"{what}: nearest d^2 error {err:.3e} = {err / b:.3g} bars; {wrong} of {len(hits)} counts differ")
        assert count.dtype == torch.int32 and mind2.dtype == torch.float64 and count.shape == mind2.shape == (len(hits),)
        assert err <= b and wrong == 0
        again = ops.manifold_cross(q, a, dev(rad))
        assert torch.equal(again[0], count) and torch.equal(again[1], mind2), "two runs differ"
        for chunks in (1, 2, 1000):
            other = ops.manifold_cross(q, a, dev(rad), chunks=chunks)
            assert torch.equal(other[0], count) and torch.equal(other[1], mind2), f"the plan with {chunks} chunks differs"


# ---- 4. the four estimates ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=IDS)
def test_prdc(ops, i):
    Rr, G, k, ref = R.case(i)
    b = fair(Rr.shape[1], ref, IDS[i])
    assert all(0.0 < ref[n] < 1.0 or n == "density" or (n == "coverage" and i == 2) for n in R.SCALARS)
    assert ref["density"] > 0.0 and ref["density"] != 1.0
    r, g = dev(Rr), dev(G)
    out = ops.manifold_prdc(r, g, k=k)
    print("device: " + ", ".join(f"{n} {out[n]:.6g}" for n in R.SCALARS))
    for n in R.SCALARS:
        assert isinstance(out[n], float) and out[n] == ref[n], n
    for n in ("hit_real", "hit_fake"):
        assert np.array_equal(out[n].cpu().numpy(), ref[n]), n
    for n in ("near_real", "rad2_real", "rad2_fake"):
        assert float(np.abs(out[n].cpu().numpy() - ref[n]).max()) <= b, n
    # the same numbers as the parts give
    assert torch.equal(out["rad2_real"], ops.manifold_radii(r, k)) and torch.equal(out["rad2_fake"], ops.manifold_radii(g, k))
    hit_r, _ = ops.manifold_cross(g, r, out["rad2_real"])
    hit_g, near_r = ops.manifold_cross(r, g, out["rad2_fake"])
    assert torch.equal(hit_r, out["hit_real"]) and torch.equal(hit_g, out["hit_fake"]) and torch.equal(near_r, out["near_real"])
    again = ops.manifold_prdc(r, g, k=k)
    assert all(torch.equal(again[n], out[n]) if torch.is_tensor(out[n]) else again[n] == out[n] for n in out)


def test_integer_case_every_row_exact(ops):
    """small integers: every sum is exact in any order, so distances ON a sphere are ties on the device too"""
    ref = R.prdc(R.INT_REAL, R.INT_FAKE, 1)
    out = ops.manifold_prdc(dev(R.INT_REAL), dev(R.INT_FAKE), k=1)
    for n in ("hit_real", "hit_fake", "near_real", "rad2_real", "rad2_fake"):
        assert np.array_equal(out[n].cpu().numpy(), ref[n]), n
    assert [out[n] for n in R.SCALARS] == [0.8, 1.0, 1.6, 1.0]
    assert out["rad2_real"].tolist() == [4, 4, 4, 4, 18] and out["hit_real"].tolist() == [2, 3, 2, 0, 1]


def test_a_set_against_itself_and_far_sets(ops):
    Rr, G, k, _ = R.case(2)
    same = ops.manifold_prdc(dev(Rr), dev(Rr), k=k)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["density"] >= 1.0
    assert float(same["near_real"].max()) <= R.bar(Rr.shape[1], float(R.sqnorms(Rr).max())) and float(same["near_real"].min()) >= 0.0
    far = ops.manifold_prdc(dev(Rr), dev(G + np.float32(1e3)), k=k)
    assert [far[n] for n in R.SCALARS] == [0.0, 0.0, 0.0, 0.0]
    swapped, out = ops.manifold_prdc(dev(G), dev(Rr), k=k), ops.manifold_prdc(dev(Rr), dev(G), k=k)
    assert swapped["recall"] == out["precision"] and swapped["precision"] == out["recall"]
    assert torch.equal(swapped["hit_fake"], out["hit_real"])


# ---- 5. limits --------------------------------------------------------------------------------------------------------------------------
def test_limits_raise_and_write_nothing(ops):
    from multimodal_vae_comparison_amd import hipops as H
    for bad, k in ((torch.ones(4, 2049, device=DEV), 1), (torch.ones(20, 4, device=DEV), 17), (torch.ones(5, 4, device=DEV), 5),
                   (torch.ones(16385, 2, device=DEV), 1)):
        with pytest.raises(ValueError, match="MI355X path"):
            ops.manifold_radii(bad, k)
        with pytest.raises(ValueError, match="MI355X path"):
            ops.manifold_prdc(bad, bad, k=k)
    with pytest.raises(ValueError, match="MI355X path"):
        ops.manifold_cross(torch.ones(4, 2049, device=DEV), torch.ones(4, 2049, device=DEV),
                           torch.ones(4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="MI355X path"):
        ops.manifold_cross(torch.ones(4, 2, device=DEV), torch.ones(16385, 2, device=DEV),
                           torch.ones(16385, dtype=torch.float64, device=DEV))
    # the C entry points refuse the same shapes themselves and leave their outputs alone
    x = torch.ones(64, 64, device=DEV)
    n2 = torch.full((20000,), -1.0, dtype=torch.float64, device=DEV)
    rad = torch.full((20000,), -2.0, dtype=torch.float64, device=DEV)
    near = torch.full((20000,), -3.0, dtype=torch.float64, device=DEV)
    cnt = torch.full((20000,), -4, dtype=torch.int32, device=DEV)
    ws = torch.full((1 << 16,), -5.0, dtype=torch.float64, device=DEV)
    L, s = H.lib(), H.stream()
    p = H.ptr
    U = H.ERR_UNSUPPORTED
    for rows, F in ((4, 2049), (16385, 2), (0, 4)):
        assert L.mmvae_manifold_sqnorms(p(x), p(n2), rows, F, s) == U
    for rows, F, k, chunks in ((4, 2049, 1, 0), (20, 4, 17, 0), (20, 4, 0, 0), (5, 4, 5, 0), (16385, 2, 1, 0), (20, 4, 1, -1)):
        assert L.mmvae_manifold_radii(p(x), p(n2), p(ws), p(rad), rows, F, k, chunks, s) == U
    for rb, ra, F in ((4, 4, 2049), (16385, 4, 2), (4, 16385, 2), (0, 4, 2), (4, 0, 2)):
        assert L.mmvae_manifold_cross(p(x), p(n2), p(x), p(n2), p(rad), p(ws), p(cnt), p(near), rb, ra, F, 0, s) == U
    assert L.mmvae_manifold_cross(p(x), p(n2), p(x), p(n2), p(rad), p(ws), p(cnt), p(near), 4, 4, 2, -1, s) == U
    torch.cuda.synchronize()
    assert bool((n2 == -1.0).all()) and bool((rad == -2.0).all()) and bool((near == -3.0).all())
    assert bool((cnt == -4).all()) and bool((ws == -5.0).all())
    # values that are not finite and mismatched shapes: refused before a launch
    bad = torch.ones(6, 4, device=DEV)
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        ops.manifold_prdc(torch.ones(6, 4, device=DEV), bad, k=2)
    with pytest.raises(ValueError, match="one squared radius per manifold row"):
        ops.manifold_cross(x, x, rad[:63])


# ---- 6. the metric end to end -----------------------------------------------------------------------------------------------------------
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


def _check(got, real, gen, k, what):
    """the restatement on the feature rows rebuilt by hand, its margin asserted, then exact equality -> its four scalars"""
    X, Y = real.cpu().numpy(), gen.cpu().numpy()
    assert X.dtype == np.float32 and Y.dtype == np.float32
    ref = R.prdc(X, Y, k)
    fair(X.shape[1], ref, what)
    assert set(got) == set(R.SCALARS)
    for n in R.SCALARS:
        assert isinstance(got[n], float) and got[n] == ref[n], (what, n, got[n], ref[n])
    return tuple(ref[n] for n in R.SCALARS)


def _told_apart(expected):
    """the sets of one modality must not be interchangeable: {set: the restatement's four scalars} pairwise different, and
    in every set some scalar strictly between 0 and 1 -- else a result filed under the wrong key would pass"""
    values = list(expected.values())
    assert len(set(values)) == len(values), f"two sets give the same four numbers: {expected}: choose another seed"
    assert all(any(0.0 < v < 1.0 for v in four) for four in values), f"a set gives only 0s and 1s: {expected}: choose another seed"


def _decoded(model, m, like, seed, channels_last=False):
    """`real` images of modality m that lie where the model generates: decodings of seeded prior latents, shaped as `like`
    (N,C,H,W).  (An untrained decoder's outputs are far from any synthetic batch: every estimate would be 0 or 1 for every
    set.)  `channels_last`: the SVHN decoder permutes its output to (N,H,W,C), as the reference's does; the CdSprites
    image decoder only relabels its (N,C,H,W) memory."""
    g = torch.Generator().manual_seed(seed)
    loc, scale = model.pz_params
    z = (loc + scale * torch.randn(len(like), model.n_latents, generator=g).to(DEV)).unsqueeze(0).contiguous()
    with torch.no_grad():
        out = model.vaes[m].dec({"latents": z, "masks": None})[0].detach()
    if channels_last:
        out = out.reshape(len(like), *out.shape[-3:]).permute(0, 3, 1, 2)
    return out.reshape(like.shape).contiguous().clone()


CD_SEEDS = {"mopoe": 21, "poe": 21}


def _cdsprites_case(mixing, seed):
    """-> (trainer, extractor, two batches whose images are decoded prior latents, eps, joint_eps)"""
    from multimodal_vae_comparison_amd import coherence as coh
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    B, D, NJ = 6, 8, 8
    torch.manual_seed(seed)
    cfg, dims = config_from_mods(mixing, CD_MODS, D, batch_size=B)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0")
    tr.model.eval()
    torch.manual_seed(seed + 1)
    trunk = coh.attribute_features(coh.AttributeClassifier(3).to(DEV))
    batches = [cdsprites_batch(B, 6, seed=s, device=DEV) for s in (3, 4)]
    batches = [dict(b, mod_1=dict(b["mod_1"], data=_decoded(tr.model, "mod_1", b["mod_1"]["data"], seed + 10 + i)))
               for i, b in enumerate(batches)]
    # the untrained trunk maps every decoded image to nearly the same 512 values (a small spread on a common offset); the
    # extractor handed to the metric is centred on the first batch's mean, so that the rounding bar, which goes with
    # max |x|^2, is that of the spread and not of the common offset
    centre = trunk(batches[0]["mod_1"]["data"]).mean(0, keepdim=True)

    def extract(x):
        return trunk(x) - centre
    g = torch.Generator().manual_seed(seed + 2)
    eps = [torch.randn(B, D, generator=g) for _ in range(32)]      # more than the four forward() calls draw
    return tr, extract, batches, eps, torch.randn(NJ, D, generator=g)


def _cdsprites_sets(model, extract, batches, eps, joint_eps):
    """the feature sets rebuilt by hand through eps_override -> {"real", "recon", "cross", "joint"}"""
    B = len(batches[0]["mod_1"]["data"])
    with torch.no_grad():
        model.eps_override = [e.clone() for e in eps]
        real, recon, cross = [], [], []
        for b in batches:
            real.append(extract(b["mod_1"]["data"]))
            recon.append(extract(model.forward(b).mods["mod_1"].decoder_dist.loc)[:B])
            cross.append(extract(model.forward(model._given_only(b, ["mod_2"])).mods["mod_1"].decoder_dist.loc)[:B])
        model.eps_override = None
        loc, scale = model.pz_params
        zj = (loc + scale * joint_eps.to(DEV)).unsqueeze(0).contiguous()
        joint = extract(model.vaes["mod_1"].dec({"latents": zj, "masks": None})[0])
    return {"real": torch.cat(real), "recon": torch.cat(recon), "cross": torch.cat(cross), "joint": joint}


@pytest.mark.parametrize("mixing", ["mopoe", "poe"])
def test_manifold_metrics_end_to_end(hip_lib, mixing):
    B, NJ, K = 6, 8, 3
    tr, extract, batches, eps, joint_eps = _cdsprites_case(mixing, CD_SEEDS[mixing])
    model = tr.model
    model.objective(batches[0])["loss"].backward()      # a gradient to watch
    torch.cuda.synchronize()
    before = _state(model)

    out = tr.manifold_metrics(batches, {"mod_1": extract}, k=K, n_joint=NJ, eps=[e.clone() for e in eps],
                              joint_eps=joint_eps.clone())
    torch.cuda.synchronize()
    _same_state(before, _state(model))
    assert model.eps_override is None and model._eval_draws is False and torch.is_grad_enabled()
    r = out["mod_1"]
    assert set(out) == {"mod_1"} and (r["n"], r["F"], r["k"]) == (2 * B, 512, K) and set(r["cross"]) == {"mod_2"}

    sets = _cdsprites_sets(model, extract, batches, eps, joint_eps)
    assert sets["real"].shape == (2 * B, 512) and sets["recon"].shape == sets["cross"].shape == (2 * B, 512)
    assert sets["joint"].shape == (NJ, 512)
    expected = {"recon": _check(r["recon"], sets["real"], sets["recon"], K, f"{mixing} recon"),
                "from_mod_2": _check(r["cross"]["mod_2"], sets["real"], sets["cross"], K, f"{mixing} from mod_2"),
                "joint": _check(r["joint"], sets["real"], sets["joint"], K, f"{mixing} joint")}
    _told_apart(expected)
    logged = {key: float(v) for key, v in tr.logged.items() if key.startswith(tuple(f"test_{n}_" for n in R.SCALARS))}
    assert logged == {f"test_{n}_mod_1_{tag}": four[i] for tag, four in expected.items() for i, n in enumerate(R.SCALARS)}
    _same_state(before, _state(model))


MS_SEED = 31


def _digits_case(seed):
    """-> (model, {modality: extractor}, one batch whose images are decoded prior latents, eps, joint_eps)"""
    from multimodal_vae_comparison_amd import coherence as coh
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import MS_MODS, config_from_mods, mnist_svhn_batch
    B, D, NJ = 6, 8, 16
    torch.manual_seed(seed)
    cfg, dims = config_from_mods("moe", MS_MODS, D, batch_size=B)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    nets = {}
    for i, kind in enumerate(("mnist", "svhn")):
        nets[kind] = coh.DigitClassifier(kind)
        nets[kind].load_state_dict({n: (3.0 * v if n.endswith("weight") else v) for n, v in DR.default_init(kind, 50 + i).items()})
        nets[kind].to(DEV)
    batch = mnist_svhn_batch(B, seed=5, device=DEV)
    batch = {m: dict(v, data=_decoded(model, m, v["data"], seed + 10 + i, channels_last=m == "mod_2"))
             for i, (m, v) in enumerate(batch.items())}
    g = torch.Generator().manual_seed(seed + 2)
    eps = [torch.randn(B, D, generator=g) for _ in range(32)]
    return model, {"mod_1": nets["mnist"].features, "mod_2": nets["svhn"].features}, batch, eps, torch.randn(NJ, D, generator=g)


def _digits_sets(model, feats, batch, eps, joint_eps):
    """-> {modality: {"real", "recon", "cross", "joint"}} rebuilt by hand through eps_override"""
    B = len(batch["mod_1"]["data"])
    with torch.no_grad():
        model.eps_override = [e.clone() for e in eps]
        full = model.forward(batch)
        given = {"mod_1": model.forward(model._given_only(batch, ["mod_1"])),
                 "mod_2": model.forward(model._given_only(batch, ["mod_2"]))}
        model.eps_override = None
        loc, scale = model.pz_params
        zj = (loc + scale * joint_eps.to(DEV)).unsqueeze(0).contiguous()
        return {m: {"real": f(batch[m]["data"]), "recon": f(full.mods[m].decoder_dist.loc)[:B],
                    "cross": f(given[other].mods[m].decoder_dist.loc)[:B],
                    "joint": f(model.vaes[m].dec({"latents": zj, "masks": None})[0])}
                for m, other, f in (("mod_1", "mod_2", feats["mod_1"]), ("mod_2", "mod_1", feats["mod_2"]))}


def test_manifold_metrics_mnist_svhn(hip_lib):
    B, NJ, K = 6, 16, 3
    model, feats, batch, eps, joint_eps = _digits_case(MS_SEED)
    out = model.manifold_metrics([batch], feats, k=K, n_joint=NJ, eps=[e.clone() for e in eps], joint_eps=joint_eps.clone())
    assert set(out) == {"mod_1", "mod_2"} and all((r["F"], r["n"], r["k"]) == (50, B, K) for r in out.values())
    assert set(out["mod_1"]["cross"]) == {"mod_2"} and set(out["mod_2"]["cross"]) == {"mod_1"}
    sets = _digits_sets(model, feats, batch, eps, joint_eps)
    expected = {}
    for m, other in (("mod_1", "mod_2"), ("mod_2", "mod_1")):
        s = sets[m]
        expected[m] = {"recon": _check(out[m]["recon"], s["real"], s["recon"], K, f"{m} recon"),
                       "cross": _check(out[m]["cross"][other], s["real"], s["cross"], K, f"{m} from {other}"),
                       "joint": _check(out[m]["joint"], s["real"], s["joint"], K, f"{m} joint")}
        _told_apart(expected[m])
    assert set(expected["mod_1"].values()) != set(expected["mod_2"].values()), "the two modalities are interchangeable"
