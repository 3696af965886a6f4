"""The mmJSD mixer (models/mmvae_models.py: MMJSD, `mixing: mmjsd`) on the GPU.

1. The objective against a composed restatement: the model's own encoders and decoders, but the dynamic prior, the KL
   rows, the per-row expert selection (tests/js_reference.py in float32 on the device) and the loss assembly in plain
   torch ops, on three models -- the CdSprites+ towers (B = 5, T = 6, D = 8), MNIST + SVHN (B = 5, D = 8), image + text +
   actions (B = 4, T = 5, D = 8: three experts) -- with a likelihood scale per modality, for prior_weight in {0.2,
   1 / (M + 1), 0.6} x beta in {1, 2.5} with recorded noise.  loss, kld, kld_prior, kld_experts and every reconstruction
   sum at 1e-4 relative (the end-to-end bar of test_parity_e2e.py), every parameter gradient at 1e-4 of its tensor's
   maximum.  Train mode: the towers without dropout (MNIST + SVHN) are compared as in eval mode; the towers with dropout
   draw other masks in every pass, so there the returned terms are held to the loss formula instead.
2. The captured step (trainer.capture / fused_step) on two towers and on three, and with the side stream disabled.
3. The evaluation metrics reach the mixer: they are MOE's.

Worst measured on an MI355X (printed with -s): loss and KL terms 2.3e-7 relative, parameter gradients 1.5e-6 of their
tensor's maximum (the image encoder's logvar bias on the CdSprites+ towers, the prior parameter on MNIST + SVHN)."""
import math

import pytest
import torch

import js_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BETAS = (1.0, 2.5)
ACT = {"enc": "Transformer", "dec": "Transformer", "data_dim": [6, 4, 1], "ltype": "optimal_sigma"}
_MODELS = {}


def _to_dev(batch):
    return {k: {kk: (vv.to(DEV) if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in batch.items()}


def _model(kind):
    """(trainer, batch on the device, recorded noise) of one of the three small models: built once"""
    if kind not in _MODELS:
        from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
        from multimodal_vae_comparison_amd.synthetic import (CD_MODS, MS_MODS, cdsprites_batch, config_from_mods,
                                                             mnist_svhn_batch, vilanro_batch)
        if kind == "cdsprites":
            mods, batch = CD_MODS, cdsprites_batch(5, 6, seed=2)
        elif kind == "mnist_svhn":
            mods, batch = MS_MODS, mnist_svhn_batch(5, seed=2)
        else:
            mods, batch = CD_MODS + [ACT], vilanro_batch(4, 5, 6, seed=2)
        # (a likelihood scale per modality: the weights of the loss assembly must pick up the right one)
        mods = [dict(m, llik_scaling=s) for m, s in zip(mods, (1.0, 2.0, 0.5))]
        cfg, dims = config_from_mods("mmjsd", mods, 8, batch_size=5, lr=1e-3)
        torch.manual_seed(0)
        tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
        tr.configure_optimizers()
        B = next(iter(batch.values()))["data"].shape[0]
        eps = torch.randn(B, 8, generator=torch.Generator().manual_seed(6))
        _MODELS[kind] = (tr, _to_dev(batch), eps)
    return _MODELS[kind]


def _has_dropout(model):
    return any(getattr(part, "drop_state", None) is not None for v in model.vaes.values() for part in (v.enc, v.dec))


def _prior_weights(M):
    return (0.2, 1.0 / (M + 1), 0.6)


def _restated(model, batch, eps, w, beta):
    """the objective from the model's own towers with the latent side and the assembly in plain torch ops"""
    from multimodal_vae_comparison_amd.models.objectives import recon_rowsum
    names = list(model.vaes.keys())
    M = len(names)
    packed = [torch.cat(model.vaes[n].enc(batch[n]), -1) for n in names]
    B = packed[0].shape[0]
    pi = [(1.0 - w) / M] * M + [w]
    _, kl, z = R.js_reference(model._pz_params[1], packed, eps.to(DEV), R.chunks(B, M).to(DEV), pi)
    recs = []
    for n in names:
        vae = model.vaes[n]
        out, _ = vae.dec({"latents": z.unsqueeze(0), "masks": batch[n]["masks"]})
        recs.append(recon_rowsum(vae.ltype, out, batch[n]).sum())
    kld_prior, kld_experts = kl[M].sum(), kl[:M].sum() / M
    kld = sum(p * kl[j].sum() for j, p in enumerate(pi))
    loss = sum(float(model.vaes[n].llik_scaling) * r for n, r in zip(names, recs)) + beta * kld
    return {"loss": loss, "kld": kld, "kld_prior": kld_prior, "kld_experts": kld_experts, "reconstruction_loss": recs}


def _grads(tr):
    return {k: p.grad.detach().clone() for k, p in tr.model.named_parameters() if p.requires_grad}


def _rel(a, b):
    a, b = float(a.detach()), float(b.detach())
    return abs(a - b) / max(abs(b), 1e-30)


@pytest.mark.parametrize("which", (0, 1, 2), ids=("w0.2", "uniform", "w0.6"))
@pytest.mark.parametrize("kind,train", [("cdsprites", False), ("mnist_svhn", False), ("mnist_svhn", True), ("three", False)])
def test_objective_matches_the_composed_restatement(hip_lib, kind, train, which):
    tr, batch, eps = _model(kind)
    model = tr.model
    model.train(train)
    assert not (train and _has_dropout(model)), "train-mode comparison: towers without dropout only"
    M = len(model.vaes)
    w = _prior_weights(M)[which]
    bad = []
    try:
        for beta in BETAS:
            model.prior_weight, model.obj_fn.beta = w, beta
            tr.zero_grad()
            model.eps_override = [eps.clone()]
            out = model.objective(batch)
            out["loss"].backward()
            got = _grads(tr)
            assert model.eps_override == []
            tr.zero_grad()
            ref = _restated(model, batch, eps, w, beta)
            ref["loss"].backward()
            want = _grads(tr)
            what = f"{kind} train={train} prior_weight={w:.3f} beta={beta}"
            for key in ("loss", "kld", "kld_prior", "kld_experts"):
                e = _rel(out[key], ref[key])
                print(f"{what}: {key} {float(out[key].detach()):.6f} vs {float(ref[key].detach()):.6f} rel {e:.2e}")
                if not e <= 1e-4:
                    bad.append(f"{what}: {key} {e:.2e}")
            assert len(out["reconstruction_loss"]) == M
            for i, (r, want_r) in enumerate(zip(out["reconstruction_loss"], ref["reconstruction_loss"])):
                assert not r.requires_grad
                if not _rel(r, want_r) <= 1e-4:
                    bad.append(f"{what}: reconstruction_loss[{i}] {_rel(r, want_r):.2e}")
            worst = (0.0, None)
            for k, g in want.items():
                d, top = float((got[k] - g).abs().max()), float(g.abs().max())
                e = 0.0 if d == 0.0 else d / max(top, 1e-30)
                worst = max(worst, (e, k))
                if not e <= 1e-4:
                    bad.append(f"{what}: grad {k} {e:.2e} (max |g| {top:.2e})")
            print(f"{what}: worst gradient {worst[0]:.2e} ({worst[1]})")
            assert bool(got["_pz_params.1"].any())      # the prior is one of the M + 1: its parameter always has a gradient
    finally:
        model.prior_weight, model.obj_fn.beta, model.eps_override = 1.0 / (M + 1), 1.0, None
        model.eval()
        tr.zero_grad()
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("kind", ["cdsprites", "three"])
def test_train_mode_terms_obey_the_loss_formula(hip_lib, kind):
    """towers with dropout in train mode (no two passes draw the same masks): the returned terms are finite and
    loss = sum_m llik_m rec_m + beta kld, kld = sum_e pi_e kl[e] + pi_M kl[M]"""
    tr, batch, eps = _model(kind)
    model = tr.model
    assert _has_dropout(model)
    M = len(model.vaes)
    model.train()
    try:
        model.prior_weight, model.obj_fn.beta = 0.5, 2.5
        tr.zero_grad()
        model.eps_override = [eps.clone()]
        out = model.objective(batch)
        out["loss"].backward()
        vals = {k: float(v.detach()) for k, v in out.items() if k != "reconstruction_loss"}
        recs = [float(r) for r in out["reconstruction_loss"]]
        assert all(math.isfinite(v) for v in list(vals.values()) + recs)
        # pi_e = 0.5 / M on every expert row, 0.5 on the prior's: kld = 0.5 (kld_experts + kld_prior)
        assert vals["kld"] == pytest.approx(0.5 * vals["kld_experts"] + 0.5 * vals["kld_prior"], rel=1e-5)
        lam = [float(v.llik_scaling) for v in model.vaes.values()]
        assert vals["loss"] == pytest.approx(sum(l * r for l, r in zip(lam, recs)) + 2.5 * vals["kld"], rel=1e-5)
        assert all(bool(torch.isfinite(g).all()) for g in _grads(tr).values())
    finally:
        model.prior_weight, model.obj_fn.beta, model.eps_override = 1.0 / (M + 1), 1.0, None
        model.eval()
        tr.zero_grad()


def test_every_row_is_decoded_from_its_own_expert(hip_lib):
    """sel[b] = (b M) // B reaches the kernel: with the noise at 0 the decoders' input is row b of expert sel[b]'s mean"""
    tr, batch, _ = _model("three")
    model = tr.model.eval()
    names = list(model.vaes.keys())
    seen = []
    dec = model.vaes[names[0]].dec
    orig = dec.forward
    dec.forward = lambda zd: (seen.append(zd["latents"].detach().clone()), orig(zd))[1]
    try:
        model.eps_override = [torch.zeros(4, 8)]
        with torch.no_grad():
            model.objective(batch)
            mus = [model.vaes[n].enc(batch[n])[0] for n in names]
    finally:
        del dec.forward
        model.eps_override = None
    sel = model._selection(4, torch.device(DEV))
    assert sel.tolist() == [0, 0, 1, 2] and sel.is_cuda and model._selection(4, torch.device(DEV)) is sel
    want = torch.stack([mus[int(s)][b] for b, s in enumerate(sel.tolist())])
    assert len(seen) == 1 and torch.equal(seen[0].reshape(4, 8), want)


# ---------------------------------------------------------------------------------------------
# the captured step
# ---------------------------------------------------------------------------------------------
def _captured(mods, batch, D=16, steps=40, stream_plan=True):
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import config_from_mods
    saved, seed0 = ops.StreamPlan.enabled, DropoutState._next_seed[0]
    ops.StreamPlan.enabled = stream_plan
    try:
        torch.manual_seed(0)
        DropoutState._next_seed[0] = 0x1234567      # the towers' dropout seeds come from a process-wide sequence
        B = next(iter(batch.values()))["data"].shape[0]
        cfg, dims = config_from_mods("mmjsd", mods, D, batch_size=B, lr=1e-3)
        tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
        tr.model.train()
        tr.configure_optimizers()
        batch = _to_dev(batch)
        eager = float(tr.model.objective(batch)["loss"].detach())
        tr.flat.zero_grad()
        tr.capture(batch, world_size=1)
        # the same noise and dropout counters whichever way the step was captured
        tr.model._rng_state[1:].zero_()
        for m in tr.model.modules():
            if isinstance(m, DropoutState):
                m.state[1:].zero_()
        losses = [float(tr.fused_step()["loss"]) for _ in range(steps)]
        torch.cuda.synchronize()
        return tr, eager, losses
    finally:
        ops.StreamPlan.enabled = saved
        DropoutState._next_seed[0] = seed0


@pytest.mark.parametrize("towers", [2, 3])
def test_captured_step(hip_lib, towers):
    """trainer.capture / fused_step as test_captured_step_every_mixer builds it, on the CdSprites+ towers and on image +
    text + actions (three towers on two streams): 40 steps, finite and decreasing"""
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, vilanro_batch
    if towers == 2:
        mods, batch = CD_MODS, cdsprites_batch(32, 12, seed=2)
    else:
        mods, batch = CD_MODS + [ACT], vilanro_batch(16, 8, 6, seed=2)
    tr, eager, losses = _captured(mods, batch)
    assert math.isfinite(eager) and all(math.isfinite(v) for v in losses), (eager, losses[:5])
    assert abs(losses[0] - eager) <= 0.05 * abs(eager), (losses[0], eager)      # different noise / dropout draws
    assert min(losses[-5:]) < losses[0], (losses[0], losses[-5:])
    assert int(tr.optimizer.step_dev[0]) == 40
    for key in ("kld", "kld_prior", "kld_experts"):
        assert math.isfinite(float(tr._static_out[key]))
    assert len(tr._static_out["reconstruction_loss"]) == towers


def test_captured_two_stream_step_is_the_one_stream_step_bit_for_bit(hip_lib):
    """the side stream changes when the towers run, not what they compute: the same steps captured with StreamPlan
    disabled give identical losses and parameters"""
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch
    runs = [_captured(CD_MODS, cdsprites_batch(32, 12, seed=2), steps=3, stream_plan=plan) for plan in (True, False)]
    assert runs[0][2] == runs[1][2], (runs[0][2], runs[1][2])
    assert torch.equal(runs[0][0].flat.data, runs[1][0].flat.data)


# ---------------------------------------------------------------------------------------------
# the metrics reach it
# ---------------------------------------------------------------------------------------------
def test_metrics_reach_the_mixer(hip_lib):
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
    res = model.cross_modal_retrieval([batch], ks=(1,), keep=2)
    assert math.isfinite(res["mean"]["mean_rank"]) and f"{names[0]}->{names[1]}" in res
    ll = model.estimate_log_likelihood(batch, K=8, given=names)      # (the proposal is the mixture over both: K % 2 == 0)
    assert ll["joint"].shape == (B,) and bool(torch.isfinite(ll["joint"]).all()) and bool(torch.isfinite(ll["ess"]).all())
    rq = model.reconstruction_quality([batch])
    img = rq[names[0]]
    assert math.isfinite(img["recon"]["ssim"]) and math.isfinite(img["recon"]["mse"])
    assert math.isfinite(img["cross"][names[1]]["ssim"])
