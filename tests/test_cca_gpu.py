"""GPU tests of the cross-modal correlation (csrc/cca.hip): the fp64 product on sub-blocks, the fit,
the score kernel, the sentence features and TorchMMVAE.cross_modal_correlation end to end.  Everything is held to the
float64 restatement (tests/cca_reference.py); the bars are rounding bounds of the arithmetic, amplified by the whitening's
condition number and the values' gaps where the problem itself amplifies them (test_cca_host.py shows that the spread of the
restatement's two routes lies under them).  Nothing is held to the code under test."""
import numpy as np
import pytest
import torch

import cca_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = R.U


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


# ---- 1. the fp64 product on sub-blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3, 7), (64, 64, 4), (65, 17, 130)])
@pytest.mark.parametrize("trans", [False, True])
def test_f64_gemm_ld(ops, shape, trans):
    M, N, K = shape
    rng = np.random.RandomState(M + N + K)
    bigA, bigB = rng.standard_normal((M + 3, K + 5)), rng.standard_normal(((N if trans else K) + 2, (K if trans else N) + 7))
    scale = rng.uniform(0.5, 2.0, K)
    ra, ca, rb, cb, rc, cc = 2, 4, 1, 3, 3, 2      # where the blocks start in their matrices
    A = bigA[ra:ra + M, ca:ca + K]
    B = bigB[rb:rb + (N if trans else K), cb:cb + (K if trans else N)]
    dA, dB = dev64(bigA), dev64(bigB)
    vA, vB = dA[ra:ra + M, ca:ca + K], dB[rb:rb + B.shape[0], cb:cb + B.shape[1]]
    for sc in (None, scale):
        As = A if sc is None else A * sc
        ref = As @ (B.T if trans else B)
        bar = 4 * K * U * (np.abs(As) @ np.abs(B.T if trans else B)).max()
        runs = []
        for _ in range(2):
            bigC = torch.full((M + 5, N + 4), 7.0, dtype=torch.float64, device=DEV)
            out = ops.f64_gemm_ld(vA, vB, bigC[rc:rc + M, cc:cc + N], trans_b=trans, scale=None if sc is None else dev64(sc))
            assert out.data_ptr() == bigC[rc:rc + M, cc:cc + N].data_ptr()
            runs.append(bigC.cpu().numpy())
        got = runs[0][rc:rc + M, cc:cc + N]
        err = np.abs(got - ref).max()
        print(f"{shape} trans_b={trans} scale={'yes' if sc is not None else 'no'}: {err:.2e} (bar {bar:.2e})")
        assert err <= bar
        around = runs[0].copy()
        around[rc:rc + M, cc:cc + N] = 7.0
        assert np.all(around == 7.0), "memory around the C block was written"
        assert np.array_equal(runs[0], runs[1]), "two runs differ"
    assert torch.equal(dA, dev64(bigA)) and torch.equal(dB, dev64(bigB))


def test_f64_gemm_ld_is_f64_gemm_on_whole_matrices(ops):
    """the same tile routine: on a whole square matrix without a scale the bits are those of f64_gemm"""
    rng = np.random.RandomState(5)
    A, B = dev64(rng.standard_normal((130, 130))), dev64(rng.standard_normal((130, 130)))
    for trans in (False, True):
        assert torch.equal(ops.f64_gemm_ld(A, B, torch.empty_like(A), trans_b=trans), ops.f64_gemm(A, B, trans_b=trans))


# ---- 2. the fit ------------------------------------------------------------------------------------------------------------------------
def fit_on_device(ops, c, cuts=None):
    X = dev32(np.concatenate(c["views"], axis=1))
    st = ops.frechet_state(c["O"], DEV)
    lo = 0
    for n in cuts or [len(X)]:
        ops.frechet_update(st, X[lo:lo + n])
        lo += n
    assert lo == len(X)
    n, mu, sigma = ops.frechet_moments(st)
    assert n == c["rows"]
    return ops.cca_fit(mu, sigma, c["widths"], c["k"], R.RIDGE)


def check_fit(c, fit, what):
    O, k = c["O"], c["k"]
    values = fit["correlations"].cpu().numpy()
    P = R.align_signs(np.concatenate([p.cpu().numpy() for p in fit["projections"]], axis=0), c["P"])
    e_val, e_proj = np.abs(values - c["values"]).max(), np.abs(P - c["P"]).max()
    e_norm = np.abs(np.linalg.norm(P, axis=0) - 1.0).max()
    print(f"{what}: sweeps {fit['sweeps']}, condition {fit['condition']}; values {e_val:.2e} (bar {c['bar_values']:.2e}; the "
          f"two float64 routes {c['spread_values']:.2e}), projections {e_proj:.2e} (bar {c['bar_projections']:.2e}; "
          f"{c['spread_projections']:.2e}), unit norm {e_norm:.2e} (bar {4 * O * U:.2e})")
    assert values.shape == (k,) and P.shape == (O, k) and [p.shape[0] for p in fit["projections"]] == list(c["widths"])
    assert e_val <= c["bar_values"] and e_proj <= c["bar_projections"] and e_norm <= 4 * O * U
    assert np.all(np.diff(values) <= 0)
    for m, ref in zip(fit["means"], c["means"]):
        assert np.abs(m.cpu().numpy() - ref).max() <= 4 * c["rows"] * U * max(np.abs(v).max() for v in c["views"])
    assert np.allclose(fit["condition"], c["condition"], rtol=1e-6)
    assert len(fit["sweeps"]["views"]) == len(c["widths"]) and 1 <= fit["sweeps"]["joint"] < 30


@pytest.mark.parametrize("name", ["odd", "edge", "three"])
def test_cca_fit(ops, name):
    c = R.case(name)
    fit = fit_on_device(ops, c)
    check_fit(c, fit, name)
    # the mean score of further pairs under the device's fit against the restatement's
    cos, total = ops.cca_score(dev32(c["test"][0]), dev32(c["test"][1]), fit["means"][0], fit["means"][1],
                               fit["projections"][0], fit["projections"][1])
    bar = R.mean_score_bar(c, c["test"][0], c["test"][1])
    got = float(total) / R.SCORE_ROWS
    print(f"{name}: mean score {got:.12f}, restated {c['scores'].mean():.12f}: {abs(got - c['scores'].mean()):.2e} "
          f"(bar {bar:.2e})")
    assert abs(got - c["scores"].mean()) <= bar and np.abs(cos.cpu().numpy() - c["scores"]).max() <= bar
    again = fit_on_device(ops, c)
    assert torch.equal(again["correlations"], fit["correlations"]), "two runs differ"
    assert all(torch.equal(x, y) for x, y in zip(again["projections"], fit["projections"])), "two runs differ"
    assert again["sweeps"] == fit["sweeps"]


def test_cca_fit_from_streamed_moments(ops):
    c = R.case("stream")
    check_fit(c, fit_on_device(ops, c), "stream, one batch")
    check_fit(c, fit_on_device(ops, c, (128, 128, 44)), "stream, batches of 128, 128, 44")


# ---- 3. the score ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "edge"])
@pytest.mark.parametrize("k", [1, 4, 64])
def test_cca_score(ops, name, k):
    c = R.case(name)
    oa, ob = c["widths"]
    rng = np.random.RandomState(k)
    if k <= c["k"]:      # the fitted projections; beyond the narrowest view random unit columns
        Pa, Pb = (np.ascontiguousarray(p[:, :k]) for p in R.split(c["P"], c["widths"]))
    else:
        Pa, Pb = (p / np.linalg.norm(p, axis=0) for p in (rng.standard_normal((oa, k)), rng.standard_normal((ob, k))))
    # means a float32 row can equal: row 0 of a IS the mean, its projection is zero and the clamp makes cos = 0 exactly
    ma, mb = (m.astype(np.float32).astype(np.float64) for m in c["means"][:2])
    a_all, b_all = c["test"][0].copy(), c["test"][1].copy()
    a_all[0] = ma.astype(np.float32)
    for rows in (1, 63, 65, 200):
        a, b = a_all[:rows], b_all[:rows]
        ref, prod = R.cosine_scores(a, b, ma, mb, Pa, Pb)
        assert ref[0] == 0.0 and prod[0] < 1e-6
        bar = R.score_bar(c["spread_rows"], oa, ob, k, prod[1:] if rows > 1 else np.ones(1))
        cos, total = ops.cca_score(dev32(a), dev32(b), dev64(ma), dev64(mb), dev64(Pa), dev64(Pb))
        got = cos.cpu().numpy()
        err = np.abs(got - ref).max()
        print(f"{name} k={k} rows={rows}: {err:.2e} (bar {bar:.2e}: 8 x spread {8 * c['spread_rows']:.2e}, rounding "
              f"{4 * (oa + ob + k) * U / (prod[1:].min() if rows > 1 else 1.0):.2e})")
        assert got.shape == (rows,) and got[0] == 0.0 and err <= bar
        assert float(total) == R.fixed_order_sum(got), "the sum is not the fixed-order sum of the rows"
        cos2, total2 = ops.cca_score(dev32(a), dev32(b), dev64(ma), dev64(mb), dev64(Pa), dev64(Pb))
        assert torch.equal(cos2, cos) and torch.equal(total2, total), "two runs differ"


# ---- 4. sentence features --------------------------------------------------------------------------------------------------------------
def sentence_ids(T, rng):
    """three sentences: an eos at position 0, no eos, two eos tokens (the first counts)"""
    ids = rng.randint(3, 10, (3, T))
    ids[0, 0] = 2
    ids[2, T // 2] = 2
    ids[2, T - 1] = 2
    return ids


@pytest.mark.parametrize("T", [1, 5, 32])
@pytest.mark.parametrize("E", [3, 64, 300])
def test_sentence_features(ops, T, E):
    rng = np.random.RandomState(100 * T + E)
    ids = sentence_ids(T, rng)
    emb, w = rng.standard_normal((10, E)).astype(np.float32), rng.uniform(0.1, 1.0, 10).astype(np.float32)
    pc = rng.standard_normal(E)
    pc /= np.linalg.norm(pc)
    for given in (None, pc):
        ref = R.sentence_features(ids, emb, w, 2, given)
        got = ops.sentence_features(torch.from_numpy(ids).to(DEV), dev32(emb), dev32(w), 2,
                                    None if given is None else dev64(given))
        assert got.dtype == torch.float32 and got.shape == (3, E)
        err, bar = np.abs(got.cpu().numpy().astype(np.float64) - ref).max(), 2.0 ** -23 * np.abs(ref).max()
        print(f"T={T} E={E} pc={'yes' if given is not None else 'no'}: {err:.2e} (bar {bar:.2e})")
        assert err <= bar
        assert np.array_equal(R.sentence_features(ids[:1], emb, w, 2)[0], float(w[2]) * emb[2].astype(np.float64))
        again = ops.sentence_features(torch.from_numpy(ids).to(DEV), dev32(emb), dev32(w), 2,
                                      None if given is None else dev64(given))
        assert torch.equal(again, got)


def test_sentence_features_fit_pc(ops):
    """fit_pc is moments and an eigendecomposition of the features the kernel returned (held to float64 above): the
    component is held to the top right singular vector of those same rows, centred, in float64"""
    from multimodal_vae_comparison_amd import coherence as coh
    rng = np.random.RandomState(7)
    E, V = 12, 10
    emb = (rng.standard_normal((V, E)) + 2.0 * rng.standard_normal((V, 1)) * rng.standard_normal(E)).astype(np.float32)
    sf = coh.SentenceFeatures(dev32(emb), coh.sif_weights(rng.randint(1, 100, V)).to(DEV))
    texts = [torch.from_numpy(rng.randint(0, V, (64, 8))).to(DEV) for _ in range(3)]
    onehot = torch.nn.functional.one_hot(texts[0], V).float()
    assert torch.equal(sf(onehot), sf(texts[0])), "one-hot rows and ids give different features"
    pc = sf.fit_pc(texts).cpu().numpy()
    feats = torch.cat([sf.unprojected(t) for t in texts]).cpu().numpy()
    ref, gap = R.top_component(feats)
    err = min(np.abs(pc - ref).max(), np.abs(pc + ref).max())
    bar = 4 * E * R.EPS / gap
    print(f"fit_pc: {err:.2e} (bar {bar:.2e}, relative gap {gap:.3f})")
    assert err <= bar and abs(np.linalg.norm(pc) - 1.0) <= 4 * E * U
    after = sf(texts[0]).cpu().numpy().astype(np.float64)
    assert np.abs(after @ ref).max() <= 2.0 ** -22 * np.abs(feats).max()      # the component is gone, to fp32 rounding


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
def _state(model):
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    drops = [m.state.clone() for m in model.modules() if isinstance(m, DropoutState)]
    return model._rng_state.clone(), drops


def _same_state(a, b):
    assert torch.equal(a[0], b[0]), "the training noise state moved"
    assert len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])), "a dropout counter moved"


@pytest.mark.parametrize("mixing", ["poe", "moe"])
def test_cross_modal_correlation_end_to_end(hip_lib, mixing):
    from multimodal_vae_comparison_amd import coherence as coh
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    B, D, NJ, K, V = 16, 8, 8, 4, 27
    torch.manual_seed(41)
    cfg, dims = config_from_mods(mixing, CD_MODS, D, batch_size=B)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    g = torch.Generator().manual_seed(42)
    lin = (torch.randn(3 * 64 * 64, 12, generator=g) / 64).to(DEV)
    sf = coh.SentenceFeatures(torch.randn(V, 8, generator=g).to(DEV), (0.1 + torch.rand(V, generator=g)).to(DEV))
    dumped = {"mod_1": [], "mod_2": []}

    def image(x):
        f = x.float().reshape(x.shape[0], -1) @ lin
        dumped["mod_1"].append(f.cpu().numpy())
        return f

    def text(x):
        f = sf(x.reshape(-1, *x.shape[-2:]))
        dumped["mod_2"].append(f.cpu().numpy())
        return f

    feats = {"mod_1": image, "mod_2": text}
    fit_batches = [cdsprites_batch(B, 6, seed=s, device=DEV) for s in (3, 4, 5)]
    batches = [cdsprites_batch(B, 6, seed=s, device=DEV) for s in (6, 7)]
    eps = [torch.randn(B, D, generator=g) for _ in range(32)]
    joint_eps = torch.randn(NJ, D, generator=g)
    before = _state(model)
    out = model.cross_modal_correlation(fit_batches, batches, feats, K, n_joint=NJ, eps=[e.clone() for e in eps],
                                        joint_eps=joint_eps.clone())
    torch.cuda.synchronize()
    _same_state(before, _state(model))
    assert model.eps_override is None and model._eval_draws is False
    assert out["k"] == K and out["n_fit"] == 3 * B and out["widths"] == {"mod_1": 12, "mod_2": 8}
    assert set(out["real"]) == set(out["recon"]) == set(out["joint"]) == {("mod_1", "mod_2")}
    assert set(out["cross"]) == {("mod_1", "mod_2"), ("mod_2", "mod_1")}
    assert set(out["condition"]) == set(out["sweeps"]["views"]) == {"mod_1", "mod_2"} and len(out["correlations"]) == K
    for table in ("real", "recon", "cross", "joint"):
        assert all(np.isfinite(v) and -1.0 <= v <= 1.0 for v in out[table].values())

    # the same run on the restatement, from the features the extractors returned, in the order of the walk: the fit's
    # three batches; per scored batch real, recon, generated from mod_1 (the caption), from mod_2 (the image); the joint
    img, txt = dumped["mod_1"], dumped["mod_2"]
    assert len(img) == 3 + 2 * 3 + 1 and len(txt) == 3 + 2 * 3 + 1
    views = [np.concatenate(img[:3]), np.concatenate(txt[:3])]
    widths = (12, 8)
    mu, sigma = R.moments(views)
    v1, P1, all1 = R.route_eig(sigma, widths, K)
    v2, P2, _ = R.route_whitened(sigma, widths, K)
    P2 = R.align_signs(P2, P1)
    kap, _ = R.kappa(sigma, widths)
    c = {"O": 20, "k": K, "widths": widths, "P": P1, "means": R.split(mu, widths), "bar_values": 4 * 20 * R.EPS * kap,
         "spread_rows": 0.0}
    c["bar_projections"] = c["bar_values"] / R.min_gap(all1, K)
    print(f"{mixing}: kappa {kap:.3g}, gap {R.min_gap(all1, K):.3g}; the two float64 routes: values {np.abs(v1 - v2).max():.2e} "
          f"(bar {c['bar_values']:.2e}), projections {np.abs(P1 - P2).max():.2e} (bar {c['bar_projections']:.2e})")
    assert np.abs(v1 - v2).max() <= c["bar_values"] and np.abs(P1 - P2).max() <= c["bar_projections"]
    assert np.abs(np.array(out["correlations"]) - v1).max() <= c["bar_values"]
    Pa, Pb = R.split(P1, widths)

    def restated(fa, fb):
        s, _ = R.cosine_scores(fa, fb, c["means"][0], c["means"][1], Pa, Pb)
        return s.mean(), R.mean_score_bar(c, fa, fb)

    sets = {"real": [], "recon": [], "from_1": [], "from_2": []}
    for i in range(2):
        r_img, rec_img, gen_img = img[3 + 3 * i: 6 + 3 * i]      # the image extractor: real, recon, generated from the caption
        r_txt, rec_txt, gen_txt = txt[3 + 3 * i: 6 + 3 * i]      # the caption extractor: real, recon, generated from the image
        sets["real"].append((r_img, r_txt))
        sets["recon"].append((rec_img[:B], rec_txt[:B]))
        sets["from_1"].append((r_img, gen_txt[:B]))
        sets["from_2"].append((gen_img[:B], r_txt))
    got = {"real": out["real"][("mod_1", "mod_2")], "recon": out["recon"][("mod_1", "mod_2")],
           "from_1": out["cross"][("mod_1", "mod_2")], "from_2": out["cross"][("mod_2", "mod_1")]}
    for key, rows in sets.items():
        ref, bar = restated(np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]))
        print(f"{mixing} {key}: {got[key]:.12f}, restated {ref:.12f}: {abs(got[key] - ref):.2e} (bar {bar:.2e})")
        assert abs(got[key] - ref) <= bar
    ref, bar = restated(img[-1], txt[-1])
    assert img[-1].shape[0] == NJ and abs(out["joint"][("mod_1", "mod_2")] - ref) <= bar

    again = model.cross_modal_correlation(fit_batches, batches, feats, K, n_joint=NJ, eps=[e.clone() for e in eps],
                                          joint_eps=joint_eps.clone())
    assert again == out, "fixed eps lists: two runs differ"
    without = model.cross_modal_correlation(fit_batches, batches, feats, K, eps=[e.clone() for e in eps])
    assert "joint" not in without and without["real"] == out["real"] and without["cross"] == out["cross"]
    _same_state(before, _state(model))


# ---- 6. limits -------------------------------------------------------------------------------------------------------------------------
def test_limits_return_the_error_and_write_nothing(ops):
    from multimodal_vae_comparison_amd import hipops as H
    L, s = H.lib(), H.stream()
    d = torch.zeros(4096, dtype=torch.float64, device=DEV)
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    i = torch.zeros(4096, dtype=torch.int32, device=DEV)
    a, b, c = H.ptr(d), H.ptr(d[1024:]), H.ptr(d[2048:])
    for M, N, K, lda, ldb, ldc in ((0, 2, 2, 2, 2, 2), (2, 0, 2, 2, 2, 2), (2, 2, 0, 2, 2, 2), (2049, 2, 2, 2, 2, 2),
                                   (2, 2049, 2, 2, 2049, 2049), (2, 2, 2049, 2049, 2, 2), (2, 3, 4, 3, 3, 3),
                                   (2, 3, 4, 4, 2, 3), (2, 3, 4, 4, 3, 2)):
        assert L.mmvae_f64_gemm_ld(a, lda, b, ldb, c, ldc, None, M, N, K, 0, s) == H.ERR_UNSUPPORTED, (M, N, K, lda, ldb, ldc)
    assert L.mmvae_f64_gemm_ld(a, 4, b, 3, c, 3, None, 2, 3, 4, 1, s) == H.ERR_UNSUPPORTED      # B^T: ldb >= K
    fa, fb = H.ptr(f), H.ptr(f[2048:])
    for rows, oa, ob, k in ((0, 3, 3, 2), (4, 0, 3, 2), (4, 3, 2049, 2), (4, 3, 3, 0), (4, 3, 3, 65)):
        assert L.mmvae_cca_score(fa, fb, a, a, b, b, c, c, rows, oa, ob, k, s) == H.ERR_UNSUPPORTED, (rows, oa, ob, k)
    for B, T, E, V in ((0, 4, 4, 4), (2, 0, 4, 4), (2, 513, 4, 4), (2, 4, 0, 4), (2, 4, 1025, 4), (2, 4, 4, 0)):
        assert L.mmvae_sentence_features(H.ptr(i), fa, fa, None, fb, B, T, E, V, 2, s) == H.ERR_UNSUPPORTED, (B, T, E, V)
    torch.cuda.synchronize()
    assert float(d.abs().max()) == 0.0 and float(f.abs().max()) == 0.0
    with pytest.raises(ValueError, match="at most 2048"):
        ops.cca_fit(torch.zeros(2049, dtype=torch.float64, device=DEV),
                    torch.zeros(2049, 2049, dtype=torch.float64, device=DEV), (2048, 1), 1)
    with pytest.raises(ValueError, match=r"outside the table's \[0, 10\)"):
        ops.sentence_features(torch.full((2, 3), 10, device=DEV), torch.zeros(10, 4, device=DEV), torch.ones(10, device=DEV))
