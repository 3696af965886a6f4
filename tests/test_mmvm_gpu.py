"""The MMVM mixer (models/mmvae_models.py: MMVM, `mixing: mmvm`) on the GPU.

1. The objective against a composed restatement: the model's own encoders and decoders, but the samples, the mixture-prior
   KL estimate, the closed-form KL (tests/mixprior_reference.py in float32 on the device) and the loss assembly in plain
   torch ops, on three models -- the CdSprites+ towers (B = 5, T = 6, D = 8), MNIST + SVHN (B = 5, D = 8), image + text +
   actions (B = 5, T = 5, D = 8: three experts) -- with a likelihood scale per modality, for alpha in {1, 0.5, 0} x beta in
   {1, 2.5} with recorded noise.  loss, kld, kld_mix, kld_std, the logged own-responsibility and every reconstruction sum
   at 1e-4 relative (the end-to-end bar of test_parity_e2e.py), every parameter gradient at 1e-4 of its tensor's maximum;
   at alpha = 1 the prior parameter's gradient is exactly 0.  Train mode: the towers without dropout (MNIST + SVHN) are
   compared as in eval mode; the towers with dropout draw other masks in every pass, so there the returned terms are held
   to the loss formula instead.
2. The captured step (trainer.capture / fused_step) on two towers and on three: the eager step's loss and gradients, the
   same bits with the side stream disabled and when repeated, twenty Adam steps that lower the loss.
3. The evaluation metrics reach the mixer: they are MOE's.

Worst measured on an MI355X (printed with -s): loss, KL terms and resp_self 2.5e-7 relative; parameter gradients
1.8e-5 to 3.5e-5 of its maximum on the prior parameter at alpha < 1 (theta = 0: the softmax's backward subtracts column sums
that agree to two digits, on both sides in float32; the op against float64: 5.6e-7), every other tensor under 8e-7; resp_self of the three models 0.69 / 0.49 / 0.59; the captured step's loss
and gradients equal the eager step's bit for bit."""
import math

import pytest
import torch

import mixprior_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BETAS = (1.0, 2.5)
ALPHAS = (1.0, 0.5, 0.0)
ACT = {"enc": "Transformer", "dec": "Transformer", "data_dim": [6, 4, 1], "ltype": "optimal_sigma"}
_MODELS = {}


def _to_dev(batch):
    return {k: {kk: (vv.to(DEV) if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in batch.items()}


def _model(kind):
    """(trainer, batch on the device, recorded noise (M,B,D)) of one of the three small models: built once"""
    if kind not in _MODELS:
        from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
        from multimodal_vae_comparison_amd.synthetic import (CD_MODS, MS_MODS, cdsprites_batch, config_from_mods,
                                                             mnist_svhn_batch, vilanro_batch)
        if kind == "cdsprites":
            mods, batch = CD_MODS, cdsprites_batch(5, 6, seed=2)
        elif kind == "mnist_svhn":
            mods, batch = MS_MODS, mnist_svhn_batch(5, seed=2)
        else:
            mods, batch = CD_MODS + [ACT], vilanro_batch(5, 5, 6, seed=2)
        # (a likelihood scale per modality: the weights of the loss assembly must pick up the right one)
        mods = [dict(m, llik_scaling=s) for m, s in zip(mods, (1.0, 2.0, 0.5))]
        cfg, dims = config_from_mods("mmvm", mods, 8, batch_size=5, lr=1e-3)
        torch.manual_seed(0)
        tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
        tr.configure_optimizers()
        _pull_the_means_together(tr.model)
        B = next(iter(batch.values()))["data"].shape[0]
        eps = torch.randn(len(mods), B, 8, generator=torch.Generator().manual_seed(6))
        _MODELS[kind] = (tr, _to_dev(batch), eps)
    return _MODELS[kind]


def _pull_the_means_together(model, factor=0.05):
    """freshly initialised towers put their posteriors several scales apart (sigma is about 1 / D, the means differ by about
    0.5 a column): every responsibility is exactly 1, kl_mix is log M to the last bit and its gradient exactly 0 -- the
    comparison would pass on a regulariser that computes nothing (measured: resp_self 1.000000 on the CdSprites+ towers
    and on the three).  The mean heads are scaled down so that the posteriors overlap, as they do once the regulariser has
    pulled them together; the objective test asserts that they do."""
    with torch.no_grad():
        for v in model.vaes.values():
            head = v.enc._heads()[0]
            head.weight.mul_(factor)
            head.bias.mul_(factor)


def _has_dropout(model):
    return any(getattr(part, "drop_state", None) is not None for v in model.vaes.values() for part in (v.enc, v.dec))


def _restated(model, batch, eps, alpha, beta):
    """the objective from the model's own towers with the latent side and the assembly in plain torch ops"""
    from multimodal_vae_comparison_amd.models.objectives import recon_rowsum
    names = list(model.vaes.keys())
    M = len(names)
    packed = [torch.cat(model.vaes[n].enc(batch[n]), -1) for n in names]
    z, kl, resp = R.mixprior_reference(model._pz_params[1], packed, eps.to(DEV))
    recs = []
    for m, n in enumerate(names):      # every modality from its OWN sample
        vae = model.vaes[n]
        out, _ = vae.dec({"latents": z[m].unsqueeze(0), "masks": batch[n]["masks"]})
        recs.append(recon_rowsum(vae.ltype, out, batch[n]).sum())
    kld_mix, kld_std = kl[:M].sum(), kl[M:].sum()
    kld = alpha * kld_mix + (1.0 - alpha) * kld_std
    loss = sum(float(model.vaes[n].llik_scaling) * r for n, r in zip(names, recs)) + beta * kld
    resp_self = torch.stack([resp[m, m] for m in range(M)]).mean()
    return {"loss": loss, "kld": kld, "kld_mix": kld_mix, "kld_std": kld_std, "resp_self": resp_self,
            "reconstruction_loss": recs}


def _grads(tr):
    return {k: p.grad.detach().clone() for k, p in tr.model.named_parameters() if p.requires_grad}


def _rel(a, b):
    a, b = float(a.detach()), float(b.detach())
    return abs(a - b) / max(abs(b), 1e-30)


def _compare_grads(what, got, want, bad, bar=1e-4):
    worst = (0.0, "")
    for k, g in want.items():
        d, top = float((got[k] - g).abs().max()), float(g.abs().max())
        e = 0.0 if d == 0.0 else d / max(top, 1e-30)
        worst = max(worst, (e, k))
        if not e <= bar:
            bad.append(f"{what}: grad {k} {e:.2e} (max |g| {top:.2e})")
    print(f"{what}: worst gradient {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("alpha", ALPHAS, ids=("alpha1", "alpha0.5", "alpha0"))
@pytest.mark.parametrize("kind,train", [("cdsprites", False), ("mnist_svhn", False), ("mnist_svhn", True), ("three", False)])
def test_objective_matches_the_composed_restatement(hip_lib, kind, train, alpha):
    tr, batch, eps = _model(kind)
    model = tr.model
    model.train(train)
    assert not (train and _has_dropout(model)), "train-mode comparison: towers without dropout only"
    M = len(model.vaes)
    bad = []
    try:
        for beta in BETAS:
            model.alpha, model.obj_fn.beta = alpha, beta
            tr.zero_grad()
            model.eps_override = [eps[m].clone() for m in range(M)]
            out = model.objective(batch)
            out["loss"].backward()
            got = _grads(tr)
            assert model.eps_override == []
            tr.zero_grad()
            ref = _restated(model, batch, eps, alpha, beta)
            ref["loss"].backward()
            want = _grads(tr)
            what = f"{kind} train={train} alpha={alpha} beta={beta}"
            for key in ("loss", "kld", "kld_mix", "kld_std", "resp_self"):
                e = _rel(out[key], ref[key])
                print(f"{what}: {key} {float(out[key].detach()):.6f} vs {float(ref[key].detach()):.6f} rel {e:.2e}")
                if not e <= 1e-4:
                    bad.append(f"{what}: {key} {e:.2e}")
            assert not out["kld_mix"].requires_grad and not out["kld_std"].requires_grad and not out["resp_self"].requires_grad
            assert 0.0 < float(out["resp_self"]) < 0.9, "the posteriors do not overlap: the mixture term is not exercised"
            assert len(out["reconstruction_loss"]) == M
            for i, (r, want_r) in enumerate(zip(out["reconstruction_loss"], ref["reconstruction_loss"])):
                assert not r.requires_grad
                if not _rel(r, want_r) <= 1e-4:
                    bad.append(f"{what}: reconstruction_loss[{i}] {_rel(r, want_r):.2e}")
            _compare_grads(what, got, want, bad)
            if alpha == 1.0:      # the fixed prior is not part of the paper's objective: not a rounding of zero, zero
                assert not bool(got["_pz_params.1"].any())
            else:
                assert bool(got["_pz_params.1"].any())
    finally:
        model.alpha, model.obj_fn.beta, model.eps_override = 1.0, 1.0, None
        model.eval()
        tr.zero_grad()
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("kind", ["cdsprites", "three"])
def test_train_mode_terms_obey_the_loss_formula(hip_lib, kind):
    """towers with dropout in train mode (no two passes draw the same masks): the returned terms are finite and
    loss = sum_m llik_m rec_m + beta kld, kld = alpha kld_mix + (1 - alpha) kld_std"""
    tr, batch, eps = _model(kind)
    model = tr.model
    assert _has_dropout(model)
    M = len(model.vaes)
    model.train()
    try:
        model.alpha, model.obj_fn.beta = 0.25, 2.5
        tr.zero_grad()
        model.eps_override = [eps[m].clone() for m in range(M)]
        out = model.objective(batch)
        out["loss"].backward()
        vals = {k: float(v.detach()) for k, v in out.items() if k != "reconstruction_loss"}
        recs = [float(r) for r in out["reconstruction_loss"]]
        assert all(math.isfinite(v) for v in list(vals.values()) + recs)
        assert vals["kld"] == pytest.approx(0.25 * vals["kld_mix"] + 0.75 * vals["kld_std"], rel=1e-5)
        lam = [float(v.llik_scaling) for v in model.vaes.values()]
        assert vals["loss"] == pytest.approx(sum(l * r for l, r in zip(lam, recs)) + 2.5 * vals["kld"], rel=1e-5)
        assert all(bool(torch.isfinite(g).all()) for g in _grads(tr).values())
    finally:
        model.alpha, model.obj_fn.beta, model.eps_override = 1.0, 1.0, None
        model.eval()
        tr.zero_grad()


def test_every_modality_is_decoded_from_its_own_sample(hip_lib):
    """decoder m reads z_m = mu_m + sigma_m eps_m and nothing else: with the noise at 0 its input is expert m's mean"""
    tr, batch, _ = _model("three")
    model = tr.model.eval()
    names = list(model.vaes.keys())
    seen, origs = {}, {}
    for n in names:
        dec = model.vaes[n].dec
        origs[n] = dec.forward
        dec.forward = lambda zd, n=n: (seen.setdefault(n, []).append(zd["latents"].detach().clone()), origs[n](zd))[1]
    try:
        model.eps_override = [torch.zeros(5, 8) for _ in names]
        with torch.no_grad():
            model.objective(batch)
            mus = {n: model.vaes[n].enc(batch[n])[0] for n in names}
    finally:
        for n in names:
            del model.vaes[n].dec.forward
        model.eps_override = None
    for n in names:
        assert len(seen[n]) == 1 and torch.equal(seen[n][0].reshape(5, 8), mus[n]), n


# ---------------------------------------------------------------------------------------------
# the captured step
# ---------------------------------------------------------------------------------------------
def _zero_counters(tr):
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    tr.model._rng_state[1:].zero_()
    for m in tr.model.modules():
        if isinstance(m, DropoutState):
            m.state[1:].zero_()


def _captured(towers, steps=20, stream_plan=True, adam_in_graph=True):
    """a train-mode trainer on two or three towers: one eager step's loss and gradients, then the captured step on the same
    noise and dropout counters -> (trainer, (eager loss, eager gradients), captured losses)"""
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods, vilanro_batch
    if towers == 2:
        mods, batch = CD_MODS, cdsprites_batch(32, 12, seed=2)
    else:
        mods, batch = CD_MODS + [ACT], vilanro_batch(16, 8, 6, seed=2)
    saved, seed0 = ops.StreamPlan.enabled, DropoutState._next_seed[0]
    ops.StreamPlan.enabled = stream_plan
    try:
        torch.manual_seed(0)
        DropoutState._next_seed[0] = 0x1234567      # the towers' dropout seeds come from a process-wide sequence
        B = next(iter(batch.values()))["data"].shape[0]
        cfg, dims = config_from_mods("mmvm", mods, 16, batch_size=B, lr=1e-3)
        tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
        tr.model.train()
        tr.configure_optimizers()
        _pull_the_means_together(tr.model)      # (the mixture term's backward is part of the graph, not an exact zero)
        batch = _to_dev(batch)
        _zero_counters(tr)
        tr.zero_grad()
        out = tr.model.objective(batch)
        out["loss"].backward()
        torch.cuda.synchronize()
        eager = (float(out["loss"].detach()), _grads(tr))
        tr.flat.zero_grad()
        tr.capture(batch, world_size=1, optimizer_in_graph=adam_in_graph)
        _zero_counters(tr)      # the same noise and dropout counters as the eager step, whichever way it was captured
        if adam_in_graph:
            losses = [float(tr.fused_step()["loss"]) for _ in range(steps)]
        else:      # one replay without the optimiser step: the gradients stay readable
            tr.flat.zero_grad()
            tr._graph.replay()
            losses = [float(tr._static_out["loss"])]
        torch.cuda.synchronize()
        return tr, eager, losses
    finally:
        ops.StreamPlan.enabled = saved
        DropoutState._next_seed[0] = seed0


@pytest.mark.parametrize("towers", [2, 3])
def test_captured_step_is_the_eager_step(hip_lib, towers):
    """the replayed graph (optimiser left out, so that the gradients can be read) on the eager step's noise and dropout
    counters: the same loss to 1e-5 and every parameter gradient to 1e-4 of its tensor's maximum"""
    tr, (eager_loss, eager_grads), losses = _captured(towers, adam_in_graph=False)
    assert math.isfinite(eager_loss) and abs(losses[0] - eager_loss) <= 1e-5 * abs(eager_loss), (losses[0], eager_loss)
    bad = []
    _compare_grads(f"{towers} towers, captured against eager", _grads(tr), eager_grads, bad)
    assert not bad, "; ".join(bad)
    assert not bool(eager_grads["_pz_params.1"].any()) and not bool(tr.model._pz_params[1].grad.any())      # alpha = 1
    for key in ("kld", "kld_mix", "kld_std", "resp_self"):
        assert math.isfinite(float(tr._static_out[key]))
    assert len(tr._static_out["reconstruction_loss"]) == towers


@pytest.mark.parametrize("towers", [2, 3])
def test_captured_training_is_reproducible_and_lowers_the_loss(hip_lib, towers):
    """twenty captured Adam steps on a fixed batch: finite, the first one the eager step's loss, the loss goes down; the
    same steps captured again and captured with the side stream disabled give identical losses and parameters -- the side
    stream changes when the towers run, not what they compute"""
    runs = [_captured(towers, stream_plan=plan) for plan in (True, True, False)]
    tr, (eager_loss, _), losses = runs[0]
    assert all(math.isfinite(v) for v in losses), losses[:5]
    assert abs(losses[0] - eager_loss) <= 1e-5 * abs(eager_loss), (losses[0], eager_loss)
    assert min(losses[-5:]) < losses[0], (losses[0], losses[-5:])
    assert int(tr.optimizer.step_dev[0]) == 20
    for other in runs[1:]:
        assert other[2] == losses, (other[2], losses)
        assert torch.equal(other[0].flat.data, tr.flat.data)


# ---------------------------------------------------------------------------------------------
# the metrics reach it
# ---------------------------------------------------------------------------------------------
def test_metrics_reach_the_mixer(hip_lib):
    from multimodal_vae_comparison_amd import coherence as coh
    tr, batch, _ = _model("cdsprites")
    model = tr.model.eval()
    names = list(model.vaes.keys())
    B, D = 5, 8
    g = torch.Generator().manual_seed(3)
    # latents_for is forward()'s latent sample on the same draws, for every `given` subset and every modality: the
    # mixture's -- a present modality's own posterior, a missing one borrows the first present modality's sample
    for given in ([names[0]], [names[1]], names):
        eps = [torch.randn(B, D, generator=g) for _ in given]      # (one draw per present modality, in modality order)
        x = {m: (batch[m] if m in given else dict(batch[m], data=None)) for m in names}
        model.eps_override = [e.clone() for e in eps]
        with torch.no_grad():
            out = model.forward(x)
        assert model.eps_override == []
        for of in names:
            model.eps_override = [e.clone() for e in eps]
            z = model.latents_for(batch, given, of=of)
            model.eps_override = None
            assert z.shape == (B, D) and bool(torch.isfinite(z).all())
            assert torch.equal(out.mods[of].latent_samples["latents"].reshape(B, D), z), (given, of)
        for k, m in enumerate(given):      # MOE's reading of the head: mu + lv eps
            q = out.mods[m].encoder_dist
            assert torch.equal(out.mods[m].latent_samples["latents"].reshape(B, D), q.loc + q.scale * eps[k].to(DEV))
    cc = model.cross_coherence([batch], coh.AttributeClassifiers.for_level(3).to(DEV), 3)
    assert len(cc["text_image"]) == 2 and len(cc["image_text"]) == 3
    assert all(math.isfinite(v) and 0.0 <= v <= 100.0 for v in cc["text_image"] + cc["image_text"])
    assert len(cc["per_sample"]["text_image_strict"]) == B
    res = model.cross_modal_retrieval([batch], ks=(1,), keep=2)
    assert math.isfinite(res["mean"]["mean_rank"]) and f"{names[0]}->{names[1]}" in res
    ll = model.estimate_log_likelihood(batch, K=8, given=names)      # (the proposal is the mixture over both: K % 2 == 0)
    assert ll["joint"].shape == (B,) and bool(torch.isfinite(ll["joint"]).all()) and bool(torch.isfinite(ll["ess"]).all())
    rq = model.reconstruction_quality([batch])
    img = rq[names[0]]
    assert math.isfinite(img["recon"]["ssim"]) and math.isfinite(img["recon"]["mse"])
    assert math.isfinite(img["cross"][names[1]]["ssim"])
