"""GPU tests of the kernel inception distance (csrc/kid.hip), part by part: the three sums of every
subset on every path of the tile kernel, the chunk plans, the kernel's parameters, the diagonal as a matter of position,
ops.kernel_inception_distance, the refusals and TorchMMVAE.kernel_distances end to end.  Everything is held to the numpy
longdouble restatement (tests/kid_reference.py) within its rounding bounds, which come from the arithmetic and not from the
code under test; the integer case to equality.  No out-of-range index is ever handed to the C function."""
import numpy as np
import pytest
import torch

import kid_reference as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [f"{s[0]}x{s[1]}x{s[2]}m{s[3]}S{s[4]}" + ("same" if i == K.SAME else "") for i, s in enumerate(K.SHAPES)]


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def held(got, ref, bars, what):
    """every one of the 3 S sums within its bar_sum of the restatement -> the largest error in bars"""
    assert got.dtype == torch.float64 and tuple(got.shape) == ref["sums"].shape
    e = np.abs(got.cpu().numpy().astype(K.LD) - ref["sums"]).astype(np.float64) / bars["sum"][None, :]
    print(f"{what}: largest error of a sum {e.max():.3g} bars (bars {bars['sum']})")
    assert e.max() <= 1.0, (what, e)
    return float(e.max())


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K.SHAPES)), ids=IDS)
def test_sums(ops, i):
    X, Y, ix, iy, ref, bars = K.case(i)
    x, y, jx, jy = dev(X), dev(Y), dev(ix), dev(iy)
    got = ops.kid_sums(x, y, jx, jy)
    held(got, ref, bars, f"{IDS[i]}, {ops.H.lib().mmvae_kid_chunks(len(ix), ix.shape[1])} chunk(s)")
    assert torch.equal(ops.kid_sums(x, y, jx, jy), got), "two runs differ"
    assert torch.equal(ops.kid_sums(x, y, jx.int(), jy.int()), got), "int32 lists differ from int64 ones"


@pytest.mark.parametrize("i, plans", [(K.CHUNKED, (2, 3, 5)), (2, (1, 7)), (0, (1, 7))], ids=["five-tiles", "two-tiles", "one-tile"])
def test_chunk_plans(ops, i, plans):
    """two plans regroup fp64 sums: each is held to the restatement, not to another plan; each is reproducible bit for bit"""
    X, Y, ix, iy, ref, bars = K.case(i)
    x, y, jx, jy = dev(X), dev(Y), dev(ix), dev(iy)
    for chunks in plans:
        got = ops.kid_sums(x, y, jx, jy, chunks=chunks)
        held(got, ref, bars, f"{IDS[i]}, chunks = {chunks}")
        assert torch.equal(ops.kid_sums(x, y, jx, jy, chunks=chunks), got), f"two runs with {chunks} chunks differ"


def test_integer_case_is_exact(ops):
    """every kernel value is an integer: the sums are equal to the restatement's in any order of summation"""
    ref = K.kid(K.INT_REAL, K.INT_FAKE, 2, 5, idx=K.INT_IDX, **K.INT_KERNEL)
    got = ops.kid_sums(dev(K.INT_REAL), dev(K.INT_FAKE), dev(K.INT_IDX[0]), dev(K.INT_IDX[1]), **K.INT_KERNEL)
    assert got.tolist() == [[1108.0, 31140.0, 10641.0], [3548.0, 10668.0, 11449.0]]
    assert np.array_equal(got.cpu().numpy().astype(K.LD), ref["sums"])
    out = ops.kernel_inception_distance(dev(K.INT_REAL), dev(K.INT_FAKE), idx=(dev(K.INT_IDX[0]), dev(K.INT_IDX[1])), **K.INT_KERNEL)
    assert out["m"] == 5 and torch.equal(out["sums"], got) and float(out["mmd2"][1]) < 0.0
    # mmd2 from exact sums: every term passes a quotient and two additions, each rounding within u of a magnitude that the
    # sum of the three terms' magnitudes bounds (3 u of it; the terms cancel: the bar goes with them, not with the result),
    # and the decimal literal is within u of itself
    for v, e, (sxx, syy, sxy) in zip(out["mmd2"], (761.12, -205.12), got.tolist()):
        assert abs(float(v) - e) <= 4 * K.U * (sxx / 20 + syy / 20 + 2 * sxy / 25), (float(v), e)


@pytest.mark.parametrize("kernel", [dict(degree=1), dict(degree=2), dict(degree=8), dict(coef0=0.0), dict(gamma=0.013),
                                    dict(degree=2, gamma=-0.02, coef0=0.5)],
                         ids=["p1", "p2", "p8", "c0", "gamma", "negative-gamma"])
def test_kernel_parameters(ops, kernel):
    key = dict(dict(degree=3, gamma=None, coef0=1.0), **kernel)
    X, Y, ix, iy, ref, bars = K.case(1, key["degree"], key["gamma"], key["coef0"])
    held(ops.kid_sums(dev(X), dev(Y), dev(ix), dev(iy), **kernel), ref, bars, f"{IDS[1]} {kernel}")


# ---- 2. positions, not row identities ---------------------------------------------------------------------------------------------------
def test_a_set_against_itself_keeps_the_diagonal_in_sxy(ops):
    """X is Y and idx_x == idx_y: sxy = sxx + sum_i k(x_i, x_i) -- the cross sum holds position i == j, the within-set
    sums leave it out"""
    X, _, ix, _, _, _ = K.case(2)
    F, m = X.shape[1], ix.shape[1]
    ref = K.sums(X, X, ix, ix)
    diag = np.array([np.trace(K.gram(X[i], X[i], 3, 1.0 / F, 1.0)) for i in ix])
    assert np.all(diag > 0.01 * ref[:, 2] / m)      # (the diagonal is no rounding matter)
    x, jx = dev(X), dev(ix)
    got = ops.kid_sums(x, x, jx, jx).cpu().numpy().astype(K.LD)
    s2 = K.s2_of(X, X)
    b = [K.bar_sum(F, m, 3, 1.0 / F, 1.0, s2, n) for n in (m * (m - 1), m * m)]
    assert np.all(np.abs(got[:, 0] - ref[:, 0]) <= b[0]) and np.all(np.abs(got[:, 2] - ref[:, 2]) <= b[1])
    assert np.all(got[:, 0] == got[:, 1])
    assert np.all(np.abs(got[:, 2] - (got[:, 0] + diag)) <= b[0] + b[1])


def test_a_repeated_index_is_left_out_by_position_only(ops):
    """a caller's list that names one row twice (positions 0 and 70: two different tiles; positions 3 and 5: one tile):
    the copies meet each other as ordinary pairs, only i == j is left out"""
    X, Y, ix, iy, _, bars = K.case(2)
    rep = np.array(ix)
    rep[0, 70], rep[1, 5] = rep[0, 0], rep[1, 3]
    ref = K.kid(X, Y, len(rep), rep.shape[1], idx=(rep, iy))
    plain = K.sums(X, Y, ix, iy)
    assert np.all(np.abs(ref["sums"][:2, 0] - plain[:2, 0]) > 1e6 * bars["sum"][0])      # (the repeat shows in sxx)
    x, y = dev(X), dev(Y)
    held(ops.kid_sums(x, y, dev(rep), dev(iy)), ref, bars, "a repeated index")
    # left out by identity instead, the sums would lack the pair of copies: k(x, x) twice
    F = X.shape[1]
    twice = 2 * K.gram(X[rep[0, :1]], X[rep[0, :1]], 3, 1.0 / F, 1.0)[0, 0]
    assert twice > 1e6 * bars["sum"][0]


# ---- 3. the distance ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K.SHAPES)), ids=IDS)
def test_kernel_inception_distance(ops, i):
    X, Y, ix, iy, ref, bars = K.case(i)
    N, M, F, m, S, _, _ = K.SHAPES[i]
    x, y = dev(X), dev(Y)
    out = ops.kernel_inception_distance(x, y, subsets=S, subset_size=m, seed=K.SEED)
    assert set(out) == {"kid", "std", "mmd2", "sums", "idx_real", "idx_fake", "m"} and out["m"] == m
    assert out["idx_real"].dtype == out["idx_fake"].dtype == torch.int32 and out["idx_real"].device.type == "cuda"
    assert np.array_equal(out["idx_real"].cpu().numpy(), ix) and np.array_equal(out["idx_fake"].cpu().numpy(), iy)
    held(out["sums"], ref, bars, IDS[i])
    for n in ("kid", "std"):
        assert out[n].dtype == torch.float64 and out[n].dim() == 0 and out[n].device.type == "cuda"
    assert out["mmd2"].dtype == torch.float64 and tuple(out["mmd2"].shape) == (S,)
    e_mmd = float(np.abs(out["mmd2"].cpu().numpy().astype(K.LD) - ref["mmd2"]).max())
    e_kid, e_std = abs(float(K.LD(float(out["kid"])) - ref["kid"])), abs(float(K.LD(float(out["std"])) - ref["std"]))
    print(f"{IDS[i]}: kid {float(out['kid']):.6g} +- {float(out['std']):.3g}; errors mmd2 {e_mmd / bars['mmd']:.3g}, kid "
          f"{e_kid / bars['kid']:.3g}, std {e_std / bars['std']:.3g} of their bars")
    assert e_mmd <= bars["mmd"] and e_kid <= bars["kid"] and e_std <= bars["std"]
    if i == K.SAME:      # the unbiased estimator's negative values are kept
        assert int((ref["mmd2"] < 0).sum()) == 2
        assert torch.equal(out["mmd2"] < 0, dev(np.asarray(ref["mmd2"] < 0)))
    # the caller's lists reproduce the draw's result; another seed draws other lists
    again = ops.kernel_inception_distance(x, y, idx=(out["idx_real"], out["idx_fake"]))
    assert all(torch.equal(again[n], out[n]) for n in ("kid", "std", "mmd2", "sums", "idx_real", "idx_fake")) and again["m"] == m
    other = ops.kernel_inception_distance(x, y, subsets=S, subset_size=m, seed=K.SEED + 1)
    assert not torch.equal(other["idx_real"], out["idx_real"])


def test_subset_size_is_clipped_to_the_smaller_set(ops):
    X, Y, _, _, _, _ = K.case(1)      # 70 real rows, 45 generated ones
    out = ops.kernel_inception_distance(dev(X), dev(Y), subsets=2, subset_size=1000, seed=K.SEED)
    assert out["m"] == 45 and tuple(out["idx_real"].shape) == tuple(out["idx_fake"].shape) == (2, 45)
    assert all(sorted(r) == list(range(45)) for r in out["idx_fake"].tolist()) and int(out["idx_real"].max()) > 45
    back = ops.kernel_inception_distance(dev(Y), dev(X), subsets=2, subset_size=1000, seed=K.SEED)
    assert back["m"] == 45 and all(sorted(r) == list(range(45)) for r in back["idx_real"].tolist())
    ref = K.kid(X, Y, 2, 1000, K.SEED)
    assert ref["m"] == 45 and np.array_equal(out["idx_real"].cpu().numpy(), ref["idx_real"])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_ops_refuse_on_the_device(ops):
    """an index outside its set never reaches the C function: ValueError from the one min/max read"""
    x, y = torch.ones(6, 4, device=DEV), torch.ones(5, 4, device=DEV)
    ix = torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    calls = ops.CALLS[0]
    for who, lists in (("idx_x", lambda b: (b, ix)), ("idx_y", lambda b: (ix, b))):
        rows = 6 if who == "idx_x" else 5
        for value in (-1, rows, 2 ** 31):
            bad = ix.clone()
            bad[1, 2] = value
            with pytest.raises(ValueError, match=f"kid_sums: {who} holds row numbers"):
                ops.kid_sums(x, y, *lists(bad))
            with pytest.raises(ValueError, match="kernel_inception_distance: idx_.* holds row numbers"):
                ops.kernel_inception_distance(x, y, idx=lists(bad))
    with pytest.raises(ValueError, match="kid_sums: idx_x is .*float32"):
        ops.kid_sums(x, y, ix.float(), ix)
    with pytest.raises(ValueError, match=r"kid_sums: idx_x is \(2, 3\), idx_y \(2, 4\)"):
        ops.kid_sums(x, y, ix, torch.zeros(2, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="kid_sums: idx_x is on cpu"):
        ops.kid_sums(x, y, ix.cpu(), ix.cpu())
    nan = x.clone()
    nan[2, 1] = float("nan")
    with pytest.raises(ValueError, match="kid_sums: X holds values that are not finite"):
        ops.kid_sums(nan, y, ix, ix)
    with pytest.raises(ValueError, match="kernel_inception_distance: fake holds values that are not finite"):
        ops.kernel_inception_distance(y, nan, subsets=2)
    with pytest.raises(ValueError, match="kid_sums: idx_x is 2 subsets of m = 1 rows"):
        ops.kid_sums(x, y, ix[:, :1], ix[:, :1])
    with pytest.raises(ValueError, match="kernel_inception_distance: m = .* = 1 "):
        ops.kernel_inception_distance(x, y[:1], subsets=2)
    with pytest.raises(ValueError, match="kid_sums: X has F = 2049"):
        ops.kid_sums(torch.ones(4, 2049, device=DEV), torch.ones(4, 2049, device=DEV), ix, ix)
    for degree in (0, 9):
        with pytest.raises(ValueError, match="kid_sums: degree ="):
            ops.kid_sums(x, y, ix, ix, degree=degree)
    assert ops.CALLS[0] == calls, "a refused call reached the library"


def test_c_entry_point_refuses_and_writes_nothing(ops):
    """the limits at the C level (valid indices throughout): MMVAE_ERR_UNSUPPORTED, sums and ws untouched"""
    from multimodal_vae_comparison_amd import hipops as H
    x = torch.ones(64, 64, device=DEV)
    idx = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    sums = torch.full((4096,), -1.0, dtype=torch.float64, device=DEV)
    ws = torch.full((1 << 16,), -5.0, dtype=torch.float64, device=DEV)
    L, s, p = H.lib(), H.stream(), H.ptr
    # (rows_x, rows_y, F, S, m, degree, chunks)
    for rx, ry, F, S, m, degree, chunks in ((4, 4, 2049, 1, 4, 3, 0), (4, 4, 0, 1, 4, 3, 0), (4, 4, 2, 1, 1, 3, 0),
                                            (4, 4, 2, 1, 16385, 3, 0), (4, 4, 2, 0, 4, 3, 0), (4, 4, 2, 1025, 4, 3, 0),
                                            (4, 4, 2, 1, 4, 0, 0), (4, 4, 2, 1, 4, 9, 0), (4, 4, 2, 1, 4, 3, -1),
                                            (0, 4, 2, 1, 4, 3, 0), (4, 0, 2, 1, 4, 3, 0)):
        rc = L.mmvae_kid_sums(p(x), p(x), p(idx), p(idx), p(ws), p(sums), rx, ry, F, S, m, degree, 0.5, 1.0, chunks, s)
        assert rc == H.ERR_UNSUPPORTED, (rx, ry, F, S, m, degree, chunks, rc)
    torch.cuda.synchronize()
    assert bool((sums == -1.0).all()) and bool((ws == -5.0).all())
    # the same buffers inside the limits: written
    assert L.mmvae_kid_sums(p(x), p(x), p(idx), p(idx), p(ws), p(sums), 4, 4, 2, 1, 4, 3, 0.5, 1.0, 0, s) == 0
    torch.cuda.synchronize()
    assert sums[:3].tolist() == [12 * 8.0, 12 * 8.0, 16 * 8.0] and bool((sums[3:] == -1.0).all())      # k = (2 / 2 + 1)^3


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


def _decoded(model, m, like, seed):
    """`real` images of modality m that lie where the model generates: decodings of seeded prior latents, shaped as `like`"""
    g = torch.Generator().manual_seed(seed)
    loc, scale = model.pz_params
    z = (loc + scale * torch.randn(len(like), model.n_latents, generator=g).to(DEV)).unsqueeze(0).contiguous()
    with torch.no_grad():
        out = model.vaes[m].dec({"latents": z, "masks": None})[0].detach()
    return out.reshape(like.shape).contiguous().clone()


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
    # the untrained trunk maps every decoded image to nearly the same 512 values (a spread of 1e-6 on a common offset); the
    # extractor handed to the metric is centred on the first batch's mean and scaled by that batch's root mean square, so
    # that x . y / F is of order 1: the sets' distances then lie far above the rounding bars, which go with max |x|^2
    first = trunk(batches[0]["mod_1"]["data"])
    centre = first.mean(0, keepdim=True)
    spread = (first - centre).pow(2).mean().sqrt()

    def extract(x):
        return (trunk(x) - centre) / spread
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
def test_kernel_distances_end_to_end(ops, mixing):
    B, NJ, S, SIZE, SEED = 6, 8, 3, 10, 9
    tr, extract, batches, eps, joint_eps = _cdsprites_case(mixing, 21)
    model = tr.model
    model.objective(batches[0])["loss"].backward()      # a gradient to watch
    torch.cuda.synchronize()
    before = _state(model)

    out = tr.kernel_distances(batches, {"mod_1": extract}, subsets=S, subset_size=SIZE, seed=SEED, n_joint=NJ,
                              eps=[e.clone() for e in eps], joint_eps=joint_eps.clone())
    torch.cuda.synchronize()
    _same_state(before, _state(model))
    assert model.eps_override is None and model._eval_draws is False and torch.is_grad_enabled()
    r = out["mod_1"]
    assert set(out) == {"mod_1"} and set(r) == {"recon", "cross", "joint", "n", "F", "subsets", "m"}
    assert (r["n"], r["F"], r["subsets"]) == (2 * B, 512, S) and set(r["cross"]) == {"mod_2"}
    assert r["m"] == {"recon": SIZE, "from_mod_2": SIZE, "joint": NJ}      # (8 joint rows: the subset size is clipped)

    sets = _cdsprites_sets(model, extract, batches, eps, joint_eps)
    assert sets["real"].shape == sets["recon"].shape == sets["cross"].shape == (2 * B, 512) and sets["joint"].shape == (NJ, 512)
    expected = {}
    for tag, got, rows in (("recon", r["recon"], sets["recon"]), ("from_mod_2", r["cross"]["mod_2"], sets["cross"]),
                           ("joint", r["joint"], sets["joint"])):
        want = ops.kernel_inception_distance(sets["real"], rows, subsets=S, subset_size=SIZE, seed=SEED)
        assert set(got) == {"kid", "std"} and all(isinstance(v, float) for v in got.values())
        assert got == {"kid": float(want["kid"]), "std": float(want["std"])}, tag
        # and those numbers are the restatement's, on the rows rebuilt by hand
        X, Y = sets["real"].cpu().numpy(), rows.cpu().numpy()
        ref = K.kid(X, Y, S, SIZE, SEED)
        b = K.bar_mmd(512, ref["m"], 3, 1.0 / 512, 1.0, K.s2_of(X, Y))
        print(f"{mixing} {tag}: kid {got['kid']:.6g} +- {got['std']:.3g} (m = {ref['m']}; bar {b:.3e})")
        assert abs(got["kid"] - float(ref["kid"])) <= K.bar_kid(b, ref["mmd2"]) and abs(got["std"] - float(ref["std"])) <= 2 * b
        print(f"  std = {got['std'] / b:.3g} bars, |kid| = {abs(got['kid']) / b:.3g} bars")
        assert got["std"] > 1e3 * b, "the subsets of this set give one value to rounding: choose another seed"
        expected[tag] = (got["kid"], got["std"])
    assert len(set(expected.values())) == 3, f"two sets give the same numbers: {expected}: choose another seed"
    logged = {key: float(v) for key, v in tr.logged.items() if key.startswith("test_kid_")}
    assert logged == {f"test_{name}_mod_1_{tag}": v[i] for tag, v in expected.items() for i, name in enumerate(("kid", "kid_std"))}
    _same_state(before, _state(model))

    model.train()
    with pytest.raises(RuntimeError, match="kernel_distances needs eval mode"):
        tr.kernel_distances(batches, {"mod_1": extract}, subsets=S, subset_size=SIZE)
    model.eval()


def test_trainer_disentanglement_logs_and_returns_the_models_result(ops):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    D, sizes = 8, (6, 4)
    N = sum(sizes)
    torch.manual_seed(41)
    cfg, dims = config_from_mods("poe", CD_MODS, D, batch_size=sizes[0])
    batches = [cdsprites_batch(B, 6, seed=3 + i, device=DEV) for i, B in enumerate(sizes)]
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0")
    tr.model.eval()
    keys = list(tr.model.vaes.keys()) + ["joint"]
    labels = torch.stack([torch.arange(N) % 2, torch.arange(N) % 3], 1)
    torch.manual_seed(44)
    eps = {key: torch.randn(N, D) for key in keys}
    want = tr.model.disentanglement(batches, labels=labels, eps={k: e.clone() for k, e in eps.items()})
    assert not tr.logged
    got = tr.disentanglement(batches, labels=labels, eps={k: e.clone() for k, e in eps.items()})
    assert list(got) == list(want) == keys
    for key in keys:
        assert set(got[key]) == set(want[key]) and all(torch.equal(got[key][n], want[key][n]) for n in want[key])
    names = ("mi", "tc", "dwkl", "kl", "mig")
    assert set(tr.logged) == {f"test_{n}_{key}" for n in names for key in keys}
    assert all(torch.equal(tr.logged[f"test_{n}_{key}"], want[key][n]) for n in names for key in keys)
    tr.logged.clear()
    plain = tr.disentanglement(batches)      # without labels there is no gap to log
    assert list(plain) == keys and set(tr.logged) == {f"test_{n}_{key}" for n in names[:4] for key in keys}
