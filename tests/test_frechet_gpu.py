"""GPU tests of the Frechet distance (csrc/frechet.hip): the streaming moments, the fp64 MFMA
products, the Jacobi eigensolver, the distance, mmvae_digit_hidden and TorchMMVAE.frechet_distances end to end.  Everything
is held to the float64 restatement (tests/frechet_reference.py) and to the reference's recorded values
(tests/golden/frechet); the bars are rounding bounds of the arithmetic or, for the distance, the spread of the independent
float64 routes (test_frechet_host.py prints them).  Nothing is held to the code under test."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import digit_reference as DR
import frechet_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def fold(ops, X, cuts=None):
    F = X.shape[1]
    st = ops.frechet_state(F, DEV)
    x = torch.from_numpy(X).to(DEV)
    lo = 0
    for n in cuts or [len(X)]:
        ops.frechet_update(st, x[lo:lo + n])
        lo += n
    assert lo == len(X)
    return st


# ---- 1. moments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_moments(ops, name):
    c = R.case(name)
    for X, mu_ref, s_ref, cuts in ((c["X1"], c["mu1"], c["s1"], (128, 128, 44)), (c["X2"], c["mu2"], c["s2"], (200,))):
        N = len(X)
        # an N-term double sum of products bounded by the largest variance (Cauchy-Schwarz), margin 4; the mean likewise
        # with the largest feature value
        bar_s, bar_m = 4 * N * U * s_ref.diagonal().max(), 4 * N * U * float(np.abs(X).max())
        runs = [None] + ([list(cuts)] if name == "b" else [])
        for split in runs:
            st = fold(ops, X, split)
            n, mu, sigma = ops.frechet_moments(st)
            mu, sigma = mu.cpu().numpy(), sigma.cpu().numpy()
            em, es = np.abs(mu - mu_ref).max(), np.abs(sigma - s_ref).max()
            print(f"{name} N={N} batches {split or [N]}: mean {em:.2e} (bar {bar_m:.2e}), covariance {es:.2e} (bar {bar_s:.2e})")
            assert n == N and em <= bar_m and es <= bar_s
            assert np.array_equal(sigma, sigma.T)
            assert torch.equal(fold(ops, X, split), st), "two runs differ"


# ---- 2. the fp64 products ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 64, 130])
def test_f64_gemm(ops, F):
    rng = np.random.RandomState(F)
    A, B = rng.standard_normal((F, F)), rng.standard_normal((F, F)) + np.arange(F)[None, :] / F      # no symmetry anywhere
    for trans in (False, True):
        ref = A @ (B.T if trans else B)
        bar = 4 * F * U * (np.abs(A) @ np.abs(B.T if trans else B)).max()
        got = ops.f64_gemm(dev64(A), dev64(B), trans_b=trans)
        err = np.abs(got.cpu().numpy() - ref).max()
        print(f"F={F} trans_b={trans}: {err:.2e} (bar {bar:.2e})")
        assert err <= bar
        assert torch.equal(ops.f64_gemm(dev64(A), dev64(B), trans_b=trans), got)
    eye = np.eye(F)
    assert np.array_equal(ops.f64_gemm(dev64(eye), dev64(B)).cpu().numpy(), B)
    assert np.array_equal(ops.f64_gemm(dev64(eye), dev64(B), trans_b=True).cpu().numpy(), B.T)


# ---- 3. the eigensolver -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "c", "d", "f"])
def test_sym_eig(ops, name):
    S = R.case(name)["s1"]
    F = S.shape[0]
    ref = np.linalg.eigvalsh(S)
    lmax, bar = ref.max(), 4 * F * R.EPS
    out = ops.sym_eig(dev64(S))
    lam, V = out["values"].cpu().numpy(), out["vectors"].cpu().numpy()
    e_val = np.abs(np.sort(lam) - ref).max() / lmax
    e_orth = np.abs(V.T @ V - np.eye(F)).max()
    e_res = np.abs(S @ V - V * lam).max() / lmax
    print(f"{name} F={F}: {out['sweeps']} sweeps, counted rotations {out['rotations']}; values {e_val:.2e}, orthogonality "
          f"{e_orth:.2e}, residual {e_res:.2e} (bar {bar:.2e})")
    assert out["sweeps"] < R.MAX_SWEEPS and out["rotations"][-1] == 0 and len(out["rotations"]) == out["sweeps"]
    assert e_val <= bar and e_orth <= bar and e_res <= bar
    # the kernel's closed-form pair indices against the restatement's ordering: in the first sweep every pair of the
    # round-robin schedule is met once and counted; case a (F odd: the padding column) is small enough for the restatement
    # to run here, and there the counted rotations of EVERY sweep agree, which a different order of the pairs would not give
    if name in ("a", "c", "d"):
        _, _, sweeps_ref, counts_ref = R.jacobi(S)
        print(f"{name}: restatement {sweeps_ref} sweeps, counted rotations {counts_ref}")
        assert out["rotations"][0] == counts_ref[0]
        if name == "a":
            assert out["rotations"] == counts_ref and out["sweeps"] == sweeps_ref
    again = ops.sym_eig(dev64(S))
    assert torch.equal(again["values"], out["values"]) and torch.equal(again["vectors"], out["vectors"])
    assert again["rotations"] == out["rotations"]
    only = ops.sym_eig(dev64(S), vectors=False)
    assert only["vectors"] is None and torch.equal(only["values"], out["values"]) and only["sweeps"] == out["sweeps"]


def test_sym_eig_reports_the_cap(ops):
    S = R.case("c")["s1"]
    with pytest.raises(RuntimeError, match="no convergence"):
        ops.sym_eig(dev64(S), max_sweeps=2)


# ---- 4. the distance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_distance(ops, name):
    c = R.case(name)
    out = ops.frechet_distance(dev64(c["mu1"]), dev64(c["s1"]), dev64(c["mu2"]), dev64(c["s2"]))
    d, tr = float(out["distance"]), float(out["tr_covmean"])
    devs = {k: R.rel(d, c[k], c["scale"]) for k in ("recorded", "jacobi", "eigh", "nuclear")}
    print(f"{name}: d^2 = {d:.15g}, sweeps {out['sweeps']} (restatement {c['sweeps']}); deviation from "
          + ", ".join(f"{k} {v:.2e}" for k, v in devs.items()) + f" (bar {c['bar']:.2e})")
    assert all(1 <= s < R.MAX_SWEEPS for s in out["sweeps"])
    assert devs["recorded"] <= c["bar"] and devs["jacobi"] <= c["bar"]
    assert abs(tr - float(c["fx"]["tr_covmean"])) <= c["bar"] * (c["scale"] or max(abs(c["recorded"]), tr))
    if name == "e":
        assert abs(d) <= c["bar"] * c["scale"]
    again = ops.frechet_distance(dev64(c["mu1"]), dev64(c["s1"]), dev64(c["mu2"]), dev64(c["s2"]))
    assert torch.equal(again["distance"], out["distance"]) and again["sweeps"] == out["sweeps"]


def test_distance_from_streamed_moments(ops):
    """the whole path of case b on the device: uneven batches -> moments -> distance"""
    c = R.case("b")
    _, mu1, s1 = ops.frechet_moments(fold(ops, c["X1"], [128, 128, 44]))
    _, mu2, s2 = ops.frechet_moments(fold(ops, c["X2"]))
    d = float(ops.frechet_distance(mu1, s1, mu2, s2)["distance"])
    print(f"b, streamed: deviation from recorded {R.rel(d, c['recorded']):.2e} (bar {c['bar']:.2e})")
    assert R.rel(d, c["recorded"]) <= c["bar"] and R.rel(d, c["jacobi"]) <= c["bar"]


# ---- 5. the digit classifiers' hidden layer ----------------------------------------------------------------------------------------
def _hidden64(kind, par, x):
    p = {k: v.double() for k, v in par.items()}
    h = Fn.relu(Fn.max_pool2d(Fn.conv2d(x.double(), p["conv1.weight"], p["conv1.bias"]), 2))
    h = Fn.relu(Fn.max_pool2d(Fn.conv2d(h, p["conv2.weight"], p["conv2.bias"]), 2)).reshape(x.shape[0], DR.FLAT[kind])
    return Fn.relu(Fn.linear(h, p["fc1.weight"], p["fc1.bias"]))


@pytest.mark.parametrize("N", [3, 70])
def test_digit_hidden(ops, N):
    kinds = ("mnist", "svhn")
    par = [DR.default_init(k, 40 + i) for i, k in enumerate(kinds)]
    par = [{k: (3.0 * v if k.endswith("weight") else v) for k, v in p.items()} for p in par]
    xs = [DR.prototype_data(k, N, seed=60 + N)[0] for k in kinds]
    st = ops.digit_state(kinds, DEV, init=par)
    dx = [x.to(DEV) for x in xs]
    logp0, pred0 = ops.digit_eval(st, kinds, dx)
    hid = ops.digit_hidden(st, kinds, dx)
    logp1, pred1 = ops.digit_eval(st, kinds, dx)
    assert hid.shape == (2, N, 50) and hid.dtype == torch.float32
    assert torch.equal(logp0, logp1) and torch.equal(pred0, pred1)
    for i, k in enumerate(kinds):
        ref = _hidden64(k, par[i], xs[i])
        e = float((hid[i].cpu().double() - ref).abs().max() / ref.abs().max())
        print(f"{k} N={N}: hidden rel err {e:.3e} (bar 1e-5), {int((ref > 0).sum())} of {ref.numel()} units active")
        assert math.isfinite(e) and e <= 1e-5 and bool((ref > 0).any()) and bool((hid[i] >= 0).all())
        lref = DR.forward(k, {n: v.double() for n, v in par[i].items()}, xs[i].double())
        assert float((logp0[i].cpu().double() - lref).abs().max() / lref.abs().max()) <= 1e-5
        alone = ops.digit_hidden(st[i:i + 1, :, :ops.DIGIT_N_PARAMS[k]].contiguous(), [k], [dx[i]])
        assert torch.equal(alone[0], hid[i])
        from multimodal_vae_comparison_amd.coherence import DigitClassifier
        net = DigitClassifier(k)
        net.load_state_dict(par[i], strict=True)
        assert torch.equal(net.to(DEV).features(dx[i]), hid[i])


# ---- 6. the metric end to end ---------------------------------------------------------------------------------------------------------
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


def _by_hand(real, gen, what):
    """the restatement's two cheap routes on the features themselves (N < F: rank-deficient covariances) -> (d^2, bar)"""
    X1, X2 = real.cpu().numpy(), gen.cpu().numpy()
    (mu1, s1), (mu2, s2) = R.moments(X1), R.moments(X2)
    eigh, _ = R.distance_eigh(mu1, s1, mu2, s2)
    nuc, _ = R.distance_nuclear(X1, X2)
    bar = max(4 * R.rel(eigh, nuc), R.BAR_FLOOR)
    return eigh, nuc, bar, what


def _check(got, hand):
    eigh, nuc, bar, what = hand
    print(f"{what}: d^2 = {got:.12g}; deviation from eigh {R.rel(got, eigh):.2e}, nuclear norm {R.rel(got, nuc):.2e} "
          f"(bar {bar:.2e})")
    assert R.rel(got, eigh) <= bar and R.rel(got, nuc) <= bar


@pytest.mark.parametrize("mixing", ["mopoe", "poe"])
def test_frechet_distances_end_to_end(hip_lib, mixing):
    from multimodal_vae_comparison_amd import coherence as coh
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    B, D, NJ = 6, 8, 8
    torch.manual_seed(21)
    cfg, dims = config_from_mods(mixing, CD_MODS, D, batch_size=B)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0")
    model = tr.model
    model.eval()
    torch.manual_seed(22)
    extract = coh.attribute_features(coh.AttributeClassifier(3).to(DEV))
    batches = [cdsprites_batch(B, 6, seed=s, device=DEV) for s in (3, 4)]
    g = torch.Generator().manual_seed(23)
    eps = [torch.randn(B, D, generator=g) for _ in range(32)]      # more than the four forward() calls draw
    joint_eps = torch.randn(NJ, D, generator=g)
    model.objective(batches[0])["loss"].backward()      # a gradient to watch
    torch.cuda.synchronize()
    before = _state(model)

    out = tr.frechet_distances(batches, {"mod_1": extract}, n_joint=NJ, eps=[e.clone() for e in eps],
                               joint_eps=joint_eps.clone())
    torch.cuda.synchronize()
    _same_state(before, _state(model))
    assert model.eps_override is None and model._eval_draws is False
    r = out["mod_1"]
    assert set(out) == {"mod_1"} and r["n"] == 2 * B and r["F"] == 512 and set(r["cross"]) == {"mod_2"}
    print(f"{mixing}: sweeps {r['sweeps']}")

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
    real = torch.cat(real)
    assert real.shape == (2 * B, 512) and joint.shape == (NJ, 512)
    _check(r["recon"], _by_hand(real, torch.cat(recon), f"{mixing} recon"))
    _check(r["cross"]["mod_2"], _by_hand(real, torch.cat(cross), f"{mixing} from mod_2"))
    _check(r["joint"], _by_hand(real, joint, f"{mixing} joint"))
    assert float(tr.logged["test_frechet_mod_1_recon"]) == r["recon"]
    assert float(tr.logged["test_frechet_mod_1_from_mod_2"]) == r["cross"]["mod_2"]
    assert float(tr.logged["test_frechet_mod_1_joint"]) == r["joint"]
    _same_state(before, _state(model))


def test_frechet_distances_mnist_svhn(hip_lib):
    from multimodal_vae_comparison_amd import coherence as coh
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import MS_MODS, config_from_mods, mnist_svhn_batch
    B, D, NJ = 6, 8, 16
    torch.manual_seed(31)
    cfg, dims = config_from_mods("moe", MS_MODS, D, batch_size=B)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    nets = {}
    for i, k in enumerate(("mnist", "svhn")):
        nets[k] = coh.DigitClassifier(k)
        nets[k].load_state_dict({n: (3.0 * v if n.endswith("weight") else v) for n, v in DR.default_init(k, 50 + i).items()})
        nets[k].to(DEV)
    batch = mnist_svhn_batch(B, seed=5, device=DEV)
    g = torch.Generator().manual_seed(33)
    eps = [torch.randn(B, D, generator=g) for _ in range(32)]
    joint_eps = torch.randn(NJ, D, generator=g)
    feats = {"mod_1": nets["mnist"].features, "mod_2": nets["svhn"].features}
    out = model.frechet_distances([batch], feats, n_joint=NJ, eps=[e.clone() for e in eps], joint_eps=joint_eps.clone())
    assert set(out) == {"mod_1", "mod_2"} and all(r["F"] == 50 and r["n"] == B for r in out.values())
    assert set(out["mod_1"]["cross"]) == {"mod_2"} and set(out["mod_2"]["cross"]) == {"mod_1"}
    with torch.no_grad():
        model.eps_override = [e.clone() for e in eps]
        full = model.forward(batch)
        given1 = model.forward(model._given_only(batch, ["mod_1"]))
        given2 = model.forward(model._given_only(batch, ["mod_2"]))
        model.eps_override = None
        loc, scale = model.pz_params
        zj = (loc + scale * joint_eps.to(DEV)).unsqueeze(0).contiguous()
        for m, other, cross_out in (("mod_1", "mod_2", given2), ("mod_2", "mod_1", given1)):
            f = feats[m]
            real = f(batch[m]["data"])
            _check(out[m]["recon"], _by_hand(real, f(full.mods[m].decoder_dist.loc)[:B], f"{m} recon"))
            _check(out[m]["cross"][other], _by_hand(real, f(cross_out.mods[m].decoder_dist.loc)[:B], f"{m} from {other}"))
            _check(out[m]["joint"], _by_hand(real, f(model.vaes[m].dec({"latents": zj, "masks": None})[0]), f"{m} joint"))


# ---- 7. limits ------------------------------------------------------------------------------------------------------------------------
def test_limits_raise_and_write_nothing(ops):
    from multimodal_vae_comparison_amd import hipops as H
    with pytest.raises(ValueError, match="MI355X path"):
        ops.frechet_state(2049, DEV)
    # the C entry points refuse the same shapes themselves and leave their outputs alone
    st = torch.zeros(64, dtype=torch.float64, device=DEV)
    x = torch.ones(4, 2049, device=DEV)
    ws = torch.zeros(4096, dtype=torch.float64, device=DEV)
    L = H.lib()
    assert L.mmvae_frechet_update(H.ptr(st), H.ptr(x), H.ptr(ws), 4, 2049, H.stream()) == H.ERR_UNSUPPORTED
    sw, rot = ctypes.c_int(-1), (ctypes.c_int * 30)()
    assert L.mmvae_sym_eig(H.ptr(ws), H.ptr(ws[64:]), None, H.ptr(st), ctypes.byref(sw), rot, 2049, 30,
                           H.stream()) == H.ERR_UNSUPPORTED
    assert L.mmvae_f64_gemm(H.ptr(ws), H.ptr(ws[64:]), H.ptr(st), 2049, 0, H.stream()) == H.ERR_UNSUPPORTED
    sws = (ctypes.c_int * 2)(-1, -1)
    assert L.mmvae_frechet_distance(H.ptr(ws), H.ptr(ws), H.ptr(ws), H.ptr(ws), H.ptr(ws[64:]), H.ptr(st), sws, 2049,
                                    H.stream()) == H.ERR_UNSUPPORTED
    # n = 1: no covariance
    one = ops.frechet_state(5, DEV)
    ops.frechet_update(one, torch.ones(1, 5, device=DEV))
    with pytest.raises(ValueError, match="n >= 2"):
        ops.frechet_moments(one)
    mu = torch.zeros(5, dtype=torch.float64, device=DEV)
    sg = torch.zeros(5, 5, dtype=torch.float64, device=DEV)
    assert L.mmvae_frechet_finish(H.ptr(one), H.ptr(mu), H.ptr(sg), 1, 5, H.stream()) == H.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(st.abs().max()) == 0.0 and float(ws.abs().max()) == 0.0 and sw.value == -1 and list(sws) == [-1, -1]
    assert float(mu.abs().max()) == 0.0 and float(sg.abs().max()) == 0.0
    # NaN features and a mismatched F: refused before the state is touched
    good = fold(ops, R.case("a")["X1"])
    keep = good.clone()
    bad = torch.from_numpy(R.case("a")["X1"]).to(DEV).clone()
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        ops.frechet_update(good, bad)
    with pytest.raises(ValueError, match="the state holds floating"):
        ops.frechet_update(good, torch.ones(3, 6, device=DEV))
    with pytest.raises(ValueError, match="differ|float64"):
        ops.frechet_distance(mu, sg, mu[:4], sg[:4, :4])
    assert torch.equal(good, keep)
