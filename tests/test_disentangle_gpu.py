"""GPU tests of the latent disentanglement metrics (csrc/aggpost.hip), part by part: the joint, the
marginal and the class-conditional log-densities of the aggregate posterior, the plans, the edge cases, the limits, the
ELBO decomposition and the mutual information gap, and TorchMMVAE.disentanglement end to end.  Everything is held to the
extended-precision restatement that takes every log-sum-exp against its maximum (tests/disentangle_reference.py) and to
the rounding bar derived there, (16 * 745 + N) 2^-53 nats for a log-sum-exp output; before a case is compared, the test
asserts from the restatement alone that its numbers tell something (MI below saturation or TC away from 0, every gap
strictly inside (0, 1)).  Nothing is held to the code under test."""
import numpy as np
import pytest
import torch

import disentangle_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
LD = np.longdouble
BIG = R.CASES.index((1100, 10, 3, 5, False))


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def fair(c, what):
    """what makes the comparison worth making, from the restatement alone -> the rounding bar"""
    N, D = c["z"].shape
    e, g = c["elbo"], c["gap"]
    print(f"{what}: mi {float(e['mi']):.4f} (log N {np.log(N):.4f}), tc {float(e['tc']):.4f}, dwkl {float(e['dwkl']):.4f}, "
          f"kl {float(e['kl']):.4f}" + ("" if g is None else f", mig per factor {np.array(g['per_factor'], float).round(3)}"))
    assert abs(float(e["kl"] - (e["mi"] + e["tc"] + e["dwkl"]))) <= 1e-12
    if D <= 10:
        assert float(e["mi"]) <= 0.9 * np.log(N), "the index-code MI is saturated: choose other inputs"
    else:
        assert abs(float(e["tc"])) > 0.1, "no total correlation to measure: choose other inputs"
    if g is not None:
        assert bool(((g["per_factor"] > 0.05) & (g["per_factor"] < 0.95)).all()), "a gap at 0 or 1: choose other inputs"
    return R.bar(N)


def run(ops, c, chunks=0):
    return ops.aggregate_posterior(dev(c["z"]), dev(c["loc"]), dev(c["scale"]), laplace=c["laplace"], labels=dev(c["labels"]),
                                   chunks=chunks)


def err(got, want):
    """largest |got - want|, the difference taken in extended precision"""
    assert got.dtype == torch.float64 and tuple(got.shape) == np.shape(want), (got.dtype, got.shape, np.shape(want))
    return float(np.abs(got.cpu().numpy().astype(LD) - np.asarray(want, LD)).max())


def held(got, ref, b, what):
    """joint, marginal, conditional and self of an aggregate_posterior result against the restatement's -> worst fraction"""
    worst = 0.0
    for part in ("joint", "marginal", "conditional", "self"):
        if ref[part] is None:
            assert got[part] is None, f"{what}: a {part} without labels"
            continue
        e = err(got[part], ref[part])
        print(f"{what} {part}: error {e:.3e} = {e / b:.3g} bars (bar {b:.3e})")
        assert e <= b, (what, part, e, b)
        worst = max(worst, e / b)
    return worst


# ---- 1. the three log-sum-exp outputs, part by part ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_parts(ops, i):
    c = R.case(i)
    b = fair(c, R.IDS[i])
    got = run(ops, c)
    assert set(got) == {"joint", "marginal", "conditional", "self"}
    assert (got["conditional"] is None) == (c["labels"] is None)
    held(got, c["agg"], b, R.IDS[i])


# ---- 2. plans ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_plans(ops, i):
    c = R.case(i)
    (N, D), b = c["z"].shape, R.bar(len(c["z"]))
    plan = ops.H.lib().mmvae_aggpost_chunks(N, D)
    assert plan >= 1
    if i == BIG:
        assert plan > 1, "the default plan of the largest case must split the posterior rows"
    got, again = run(ops, c), run(ops, c)
    parts = [p for p in ("joint", "marginal", "conditional") if got[p] is not None]
    for p in parts:
        assert torch.equal(got[p], again[p]), f"two runs differ in {p}"
    for chunks in (1, 2, 3, 1000):
        other, twice = run(ops, c, chunks), run(ops, c, chunks)
        for p in parts:
            assert torch.equal(other[p], twice[p]), f"two runs with {chunks} chunks differ in {p}"
            e = float((other[p] - got[p]).abs().max())
            print(f"{R.IDS[i]} {p}: {chunks} chunks against the default plan ({plan}): {e:.3e} = {e / b:.3g} bars")
            assert e <= b, (p, chunks, e, b)
        held(other, c["agg"], b, f"{R.IDS[i]} chunks {chunks}")


# ---- 3. the edge cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["underflow", "single", "duplicate"])
def test_edge_cases(ops, name):
    c = R.special(name)
    N, D = c["z"].shape
    b = R.bar(N)
    if name == "underflow":      # (from the restatement: what the case is for)
        l = R.pair_terms(c["z"], c["loc"], c["scale"], c["laplace"])
        arg = l - l[np.arange(N), np.arange(N)][:, None, :]
        print(f"underflow: largest argument {float(arg.max()):.2f}, {float((arg < -745).mean()):.3f} of the terms below -745")
        assert float(arg.max()) > 5.0 and float((arg < -745).mean()) > 0.25
    got = run(ops, c)
    held(got, c["agg"], b, name)
    if name == "single":
        assert int(c["agg"]["counts"][0, 5]) == 1
        own = R.pair_terms(c["z"][5:6], c["loc"][5:6], c["scale"][5:6], c["laplace"])[0, 0]
        assert err(got["conditional"][0, 5], own) <= b
    if name == "duplicate":
        assert err(got["marginal"][0], c["agg"]["marginal"][1]) <= b and err(got["joint"][:1], c["agg"]["joint"][1:2]) <= b


# ---- 4. the limits ----------------------------------------------------------------------------------------------------------------------
def test_one_row_is_its_own_term(ops):
    z, loc, scale, labels = R.generate(1, 4, 2, 1, False)
    ref = R.aggregate(z, loc, scale, False, labels)
    got = ops.aggregate_posterior(dev(z), dev(loc), dev(scale), labels=dev(labels))
    b = R.bar(1)
    held(got, ref, b, "N = 1")
    own = R.pair_terms(z, loc, scale, False)[0, 0]
    assert err(got["marginal"][0], own) <= b and err(got["conditional"][0, 0], own) <= b
    assert err(got["joint"], own.sum(keepdims=True)) <= b
    out = ops.elbo_decomposition(got, dev(np.asarray(R.log_prior(z), np.float64)))
    assert abs(float(out["mi"])) <= 6 * b and abs(float(out["tc"])) <= 6 * b
    with pytest.raises(ValueError, match="single value"):
        ops.mutual_information_gap(got, dev(labels))


def test_limits_raise_and_write_nothing(ops):
    from multimodal_vae_comparison_amd import hipops as H
    ok = torch.ones(4, 3, device=DEV)
    for bad in (torch.ones(16385, 2, device=DEV), torch.ones(4, 257, device=DEV)):
        with pytest.raises(ValueError, match="MI355X path"):
            ops.aggregate_posterior(bad, bad, bad)
    with pytest.raises(ValueError, match="labels"):
        ops.aggregate_posterior(ok, ok, ok, labels=torch.zeros(9, 4, dtype=torch.int32, device=DEV))
    # the C entry point refuses the same shapes itself and leaves its outputs alone
    x = torch.ones(64, 64, device=DEV)
    lab = torch.zeros(1 << 12, dtype=torch.int32, device=DEV)
    ws = torch.full((1 << 16,), -5.0, dtype=torch.float64, device=DEV)
    joint = torch.full((20000,), -1.0, dtype=torch.float64, device=DEV)
    marg = torch.full((20000,), -2.0, dtype=torch.float64, device=DEV)
    cond = torch.full((20000,), -3.0, dtype=torch.float64, device=DEV)
    L, s, p = H.lib(), H.stream(), H.ptr
    for N, D, K, chunks in ((16385, 2, 0, 0), (4, 257, 0, 0), (4, 2, 9, 0), (0, 2, 0, 0), (4, 0, 0, 0), (4, 2, -1, 0), (4, 2, 1, -1)):
        assert L.mmvae_aggpost_lse(p(x), p(x), p(x), 0, p(lab), p(ws), p(joint), p(marg), p(cond), N, D, K, chunks, s) \
            == H.ERR_UNSUPPORTED, (N, D, K, chunks)
        assert L.mmvae_aggpost_ws_doubles(N, D, K, chunks) == 0
    assert L.mmvae_aggpost_chunks(16385, 2) == 0 and L.mmvae_aggpost_chunks(4, 257) == 0
    torch.cuda.synchronize()
    assert bool((joint == -1.0).all()) and bool((marg == -2.0).all()) and bool((cond == -3.0).all())
    assert bool((ws == -5.0).all())
    # the workspace the helper asks for is what the launch uses: the largest K, a ragged shape, more chunks than tiles
    assert L.mmvae_aggpost_ws_doubles(70, 5, 2, 0) == 70 * 5 + 70 + L.mmvae_aggpost_chunks(70, 5) * 70 * 3 * 6
    assert L.mmvae_aggpost_ws_doubles(70, 5, 2, 1000) == 70 * 5 + 70 + 3 * 70 * 3 * 6
    # values that are not finite, scales that are not positive, negative labels: refused before a launch
    bad = torch.ones(4, 3, device=DEV)
    bad[2, 1] = float("inf")
    with pytest.raises(ValueError, match="z holds values that are not finite"):
        ops.aggregate_posterior(bad, ok, ok)
    with pytest.raises(ValueError, match="scale holds values that are not positive"):
        ops.aggregate_posterior(ok, ok, ok - 1.0)
    with pytest.raises(ValueError, match="labels holds values outside"):
        ops.aggregate_posterior(ok, ok, ok, labels=torch.full((1, 4), -1, device=DEV))
    # a z that is no draw from its posterior overflows the fixed shift: said, not returned
    far = torch.zeros(2, 1, device=DEV)
    far[1, 0] = 100.0
    with pytest.raises(FloatingPointError, match="overflows"):
        ops.aggregate_posterior(far.flip(0).contiguous(), far, torch.tensor([[1.0], [0.01]], device=DEV))


# ---- 5. the scalars ---------------------------------------------------------------------------------------------------------------------
def scalars_held(ops, got, c, what, lpz=None):
    """elbo_decomposition and mutual_information_gap of the device's `got` against the restatement of case `c`"""
    N, D = c["z"].shape
    b = R.bar(N)
    lpz = dev(np.asarray(c["lpz"], np.float64)) if lpz is None else lpz
    out = ops.elbo_decomposition(got, lpz)
    assert set(out) == {"mi", "tc", "dwkl", "kl"}
    for n in ("mi", "tc", "dwkl", "kl"):
        assert out[n].dtype == torch.float64 and out[n].dim() == 0 and out[n].is_cuda
        e = abs(float(LD(float(out[n])) - c["elbo"][n]))
        print(f"{what} {n}: {float(out[n]):.12f}, error {e:.3e} = {e / ((D + 2) * b):.3g} of (D + 2) bars")
        assert e <= (D + 2) * b, (what, n, e)
    # the identity on the device's own numbers: four means of per-row float64 values, their rounding only
    size = max(float(t.abs().max()) for t in (got["self"], got["joint"], got["marginal"].sum(1), lpz))
    assert abs(float(out["kl"] - (out["mi"] + out["tc"] + out["dwkl"]))) <= 64 * R.U * max(size, 1.0)
    if c["labels"] is None:
        return out, None
    if D < 2:
        with pytest.raises(ValueError, match="D = 1"):
            ops.mutual_information_gap(got, dev(c["labels"]))
        return out, None
    gap, ref = ops.mutual_information_gap(got, dev(c["labels"])), c["gap"]
    assert set(gap) == {"mig", "per_factor", "mi", "h_z", "h_v"}
    K = len(c["labels"])
    assert gap["per_factor"].shape == (K,) and gap["mi"].shape == (K, D) and gap["h_z"].shape == (D,) and gap["h_v"].shape == (K,)
    assert err(gap["h_z"], ref["h_z"]) <= 2 * b and err(gap["mi"], ref["mi"]) <= 2 * b
    assert err(gap["h_v"], ref["h_v"]) <= 64 * R.U
    per = np.abs(gap["per_factor"].cpu().numpy().astype(LD) - ref["per_factor"]) / (4 * b / ref["h_v"])
    print(f"{what} mig: {float(gap['mig']):.12f}, per factor {float(per.max()):.3g} of 4 bars / H(v)")
    assert float(per.max()) <= 1.0
    assert abs(float(LD(float(gap["mig"])) - ref["mig"])) <= float((4 * b / ref["h_v"]).max())
    return out, gap


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_scalars(ops, i):
    c = R.case(i)
    fair(c, R.IDS[i])
    scalars_held(ops, run(ops, c), c, R.IDS[i])


def test_scalar_ops_refuse(ops):
    c = R.case(1)
    got = run(ops, c)
    with pytest.raises(ValueError, match="lpz"):
        ops.elbo_decomposition(got, torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="agg must be the dict"):
        ops.elbo_decomposition({"joint": got["joint"]}, torch.zeros(70, device=DEV))
    with pytest.raises(ValueError, match="no conditional"):
        ops.mutual_information_gap(dict(got, conditional=None), dev(c["labels"]))
    with pytest.raises(ValueError, match="factors"):
        ops.mutual_information_gap(got, dev(c["labels"][:1]))


# ---- 6. the metric end to end -----------------------------------------------------------------------------------------------------------
def _snapshot(model):
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    return [model._rng_state] + [m.state for m in model.modules() if isinstance(m, DropoutState)]


def _training_forward(model, batch):
    model.train()
    model._begin_step()
    with torch.no_grad():
        out = model.forward(batch)
    model.eval()
    torch.cuda.synchronize()
    return [out.mods[m].decoder_dist.loc.clone() for m in model.vaes] \
        + [out.mods[m].latent_samples["latents"].clone() for m in model.vaes]


@pytest.mark.parametrize("mixing", ["mopoe", "poe", "moe"])
def test_disentanglement_end_to_end(hip_lib, mixing):
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, MS_MODS, cdsprites_batch, config_from_mods, mnist_svhn_batch
    D, sizes, K = 8, (6, 4), 2
    N = sum(sizes)
    torch.manual_seed(41)
    if mixing == "moe":
        cfg, dims = config_from_mods("moe", MS_MODS, D, batch_size=sizes[0], prior="laplace")
        batches = [mnist_svhn_batch(B, seed=5 + i, device=DEV) for i, B in enumerate(sizes)]
    else:
        cfg, dims = config_from_mods(mixing, CD_MODS, D, batch_size=sizes[0])
        batches = [cdsprites_batch(B, 6, seed=3 + i, device=DEV) for i, B in enumerate(sizes)]
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    names = list(model.vaes.keys())
    keys = names + (["joint"] if mixing == "poe" else [])
    laplace = mixing == "moe"
    g = torch.Generator().manual_seed(43)
    labels = torch.stack([torch.arange(N) % 2, torch.randint(0, 3, (N,), generator=g)], 1)      # (N, K): a row per sample
    assert all(len(labels[:, k].unique()) >= 2 for k in range(K))
    draw = torch.distributions.Laplace(0.0, 1.0) if laplace else torch.distributions.Normal(0.0, 1.0)
    torch.manual_seed(44)
    eps = {key: draw.sample((N, D)) for key in keys}
    mine = model.eps_override = [torch.zeros(6, D)]
    before = [t.clone() for t in _snapshot(model)]

    out = model.disentanglement(batches, labels=labels, eps={k: e.clone() for k, e in eps.items()})
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model))), "the noise state or a dropout counter moved"
    assert model.eps_override is mine and len(mine) == 1 and model._eval_draws is False and torch.is_grad_enabled()
    model.eps_override = None
    assert list(out) == keys

    pz_loc, pz_scale = (p.detach().cpu().numpy().astype(np.float64).reshape(-1) for p in model.pz_params)
    lab = np.ascontiguousarray(labels.numpy().T.astype(np.int32))
    seen = []
    for key in keys:
        r = out[key]
        assert set(r) == {"mi", "tc", "dwkl", "kl", "mig", "per_factor", "mi_table", "h_z", "z", "loc", "scale"}
        z, loc, scale = r["z"], r["loc"], r["scale"]
        assert z.shape == loc.shape == scale.shape == (N, D) and z.dtype == loc.dtype == scale.dtype == torch.float32
        assert torch.equal(z, loc + scale * eps[key].to(DEV)), f"{key}: z is not loc + scale eps"
        zn, ln, sn = (t.cpu().numpy() for t in (z, loc, scale))
        agg = R.aggregate(zn, ln, sn, laplace and key != "joint", lab)
        ref = {"z": zn, "labels": lab, "agg": agg, "lpz": R.log_prior(zn, pz_loc, pz_scale, model.pz is torch.distributions.Laplace)}
        ref["elbo"], ref["gap"] = R.decomposition(agg, ref["lpz"]), R.gap(agg, lab)
        b = R.bar(N)
        for n in ("mi", "tc", "dwkl", "kl"):
            e = abs(float(LD(float(r[n])) - ref["elbo"][n]))
            print(f"{mixing} {key} {n}: {float(r[n]):.10f}, error {e:.3e} = {e / ((D + 2) * b):.3g} of (D + 2) bars")
            assert e <= (D + 2) * b, (key, n, e)
        assert err(r["h_z"], ref["gap"]["h_z"]) <= 2 * b and err(r["mi_table"], ref["gap"]["mi"]) <= 2 * b
        assert float((np.abs(r["per_factor"].cpu().numpy().astype(LD) - ref["gap"]["per_factor"])
                      / (4 * b / ref["gap"]["h_v"])).max()) <= 1.0
        assert abs(float(LD(float(r["mig"])) - ref["gap"]["mig"])) <= float((4 * b / ref["gap"]["h_v"]).max())
        # the ops on the tensors the call returns give the call's numbers
        again = ops.aggregate_posterior(z, loc, scale, laplace=laplace and key != "joint", labels=dev(lab))
        assert torch.equal(ops.mutual_information_gap(again, dev(lab))["mi"], r["mi_table"])
        seen.append(tuple(float(r[n]) for n in ("mi", "tc", "dwkl")))
    assert len(set(seen)) == len(seen), f"two keys give the same numbers: {seen}"
    if mixing != "moe":      # (the posterior of a modality follows its own tower)
        assert not torch.equal(out[names[0]]["loc"], out[names[1]]["loc"])

    # without labels the gap's entries are absent; without eps the draw is the evaluation generator's
    plain = model.disentanglement(batches)
    assert list(plain) == keys and all(set(r) == {"mi", "tc", "dwkl", "kl", "h_z", "z", "loc", "scale"} for r in plain.values())
    assert all(torch.equal(plain[k]["loc"], out[k]["loc"]) and not torch.equal(plain[k]["z"], out[k]["z"]) for k in keys)
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model))), "the noise state or a dropout counter moved"

    # the next training-mode forward() is the one that would have run without the call
    after_call = _training_forward(model, batches[0])
    for t, saved in zip(_snapshot(model), before):
        t.copy_(saved)
    without = _training_forward(model, batches[0])
    assert all(torch.equal(a, b) for a, b in zip(after_call, without))
