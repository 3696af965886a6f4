"""Host-side contract of the evaluation mixin (multimodal_vae_comparison_amd/models/evaluation.py) and of the helpers the
metrics share: the unimodal VAE refuses every metric by name; the noise context gives back what it found, also when the
metric raises; one place decides which generator state a draw comes from; the per-epoch permutations are the ones both
trainers used to build; coherence.py imports without the models.  The models live on the CPU: nothing here reaches a
kernel.  Numerics: test_loglik_gpu.py, test_probe_gpu.py, test_coherence_gpu.py, test_digits_gpu.py."""
import ast
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

PKG = os.path.join(ROOT, "multimodal_vae_comparison_amd")
METRICS = ("estimate_log_likelihood", "latents_for", "classify_latents", "cross_coherence", "joint_coherence",
           "digit_cross_coherence", "digit_joint_coherence")


def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


# ---- 1. the unimodal VAE's stubs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", METRICS)
def test_unimodal_vae_refuses_every_metric_by_name(name):
    from multimodal_vae_comparison_amd.models.vae import VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE)
    with pytest.raises(NotImplementedError) as e:
        getattr(vae, name)()
    text = str(e.value)
    assert "unimodal" in text and name in text and f"TorchMMVAE.{name}" in text
    if name == "estimate_log_likelihood":
        assert "poe, moe and mopoe" in text


# ---- 2. the noise context ----------------------------------------------------------------------------------------------
def _cross_call(which):
    """(model, a call of the cross-generation metric `which` on a batch that lacks a modality)"""
    from multimodal_vae_comparison_amd import coherence, synthetic
    if which == "cross_coherence":
        model = _model()
        batch = synthetic.cdsprites_batch(4, 6, seed=3)
        batch["mod_1"] = dict(batch["mod_1"], data=None)
        cls = coherence.AttributeClassifiers.for_level(3)
        return model, lambda eps: model.cross_coherence([batch], cls, 3, eps=eps)
    model = _model(mods=synthetic.MS_MODS)
    batch = synthetic.mnist_svhn_batch(4, seed=3)
    batch["mod_2"] = dict(batch["mod_2"], data=None)
    cls = coherence.DigitClassifiers()
    return model, lambda eps: model.digit_cross_coherence([(batch, torch.arange(4))], cls, eps=eps)


@pytest.mark.parametrize("which", ["cross_coherence", "digit_cross_coherence"])
@pytest.mark.parametrize("with_eps", [False, True])
def test_a_failing_cross_metric_leaves_the_noise_setup_as_it_found_it(which, with_eps):
    model, call = _cross_call(which)
    mine = model.eps_override = [torch.zeros(4, 8)]
    with pytest.raises(ValueError, match="every batch"):
        call([torch.ones(4, 8)] if with_eps else None)
    assert model._eval_draws is False
    assert model.eps_override is mine and len(mine) == 1


@pytest.mark.parametrize("fails", [False, True])
def test_latents_for_keeps_the_callers_recorded_draws(fails, monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    mine = model.eps_override = [torch.zeros(2, 8), torch.ones(2, 8)]
    seen = []

    def latents_of(x, of):
        assert model._eval_draws is True and model.eps_override is mine and not torch.is_grad_enabled()
        seen.append(of)
        if fails:
            raise KeyError(of)
        return torch.zeros(1, 2, 8)

    monkeypatch.setattr(model, "_latents_of", latents_of)
    batch = cdsprites_batch(2, 6, seed=3)
    if fails:
        with pytest.raises(KeyError):
            model.latents_for(batch, ["mod_2"])
    else:
        assert model.latents_for(batch, ["mod_2"]).shape == (2, 8)
    assert seen == ["mod_2"]
    assert model._eval_draws is False and torch.is_grad_enabled()
    assert model.eps_override is mine and len(mine) == 2


# ---- 3. which generator state a draw comes from -------------------------------------------------------------------------
def test_one_place_chooses_the_generator_state(monkeypatch):
    from multimodal_vae_comparison_amd import ops
    model = _model()
    handed = []

    def randn(shape, state):
        handed.append(state)
        return torch.zeros(shape)

    monkeypatch.setattr(ops, "randn", randn)
    cpu = torch.device("cpu")
    model._draw(2, 8, cpu)
    assert [t.shape for t in model._draw_many(3, 2, 8, cpu)] == [(2, 8)] * 3
    assert len(handed) == 2 and all(s is model._rng_state for s in handed)
    del handed[:]
    with model._eval_noise():
        assert model._eval_draws is True
        model._draw(2, 8, cpu)
        model._draw_many(3, 2, 8, cpu)
    assert len(handed) == 2 and all(s is model._eval_rng_state for s in handed)
    del handed[:]
    z = model._prior_sample(5, None, "test")       # an evaluation draw wherever it is called from
    assert z.shape == (1, 5, 8) and len(handed) == 1 and handed[0] is model._eval_rng_state
    assert model._eval_rng_state is not model._rng_state and model._eval_draws is False
    # recorded draws go round the generator in both states
    model.eps_override = [torch.ones(2, 8)] * 4
    assert len(model._draw_many(3, 2, 8, cpu)) == 3 and len(model.eps_override) == 1
    z = model._prior_sample(5, torch.ones(5, 8), "test")
    assert len(handed) == 1 and torch.equal(z, (model.pz_params[0] + model.pz_params[1]).expand(1, 5, 8))
    with pytest.raises(ValueError, match="test: n = 0"):
        model._prior_sample(0, None, "test")


# ---- 4. the per-epoch permutations ---------------------------------------------------------------------------------------
def test_epoch_orders_are_the_permutations_both_trainers_drew():
    from multimodal_vae_comparison_amd.ops import epoch_orders
    got = epoch_orders(5, 3, 7, "cpu")
    g = torch.Generator().manual_seed(7)
    want = torch.stack([torch.randperm(5, generator=g) for _ in range(3)])
    assert got.dtype == torch.int32 and got.shape == (3, 5) and got.device.type == "cpu"
    assert torch.equal(got.long(), want)
    assert all(sorted(row) == list(range(5)) for row in got.tolist())
    assert epoch_orders(5, 3, 7, "cpu", shuffle=False) is None


# ---- 5. who imports whom ---------------------------------------------------------------------------------------------
def test_coherence_imports_without_the_models():
    code = ("import sys; import multimodal_vae_comparison_amd.coherence; "
            "bad = [m for m in sys.modules if m.startswith('multimodal_vae_comparison_amd.models')]; "
            "assert not bad, bad")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


@pytest.mark.parametrize("path", ["coherence.py", "models/evaluation.py", "models/mmvae_base.py"])
def test_no_import_hides_inside_a_function(path):
    with open(os.path.join(PKG, path)) as f:
        tree = ast.parse(f.read())
    inner = [n.lineno for fn in ast.walk(tree) if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef))
             for n in ast.walk(fn) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert not inner, f"{path}: imports inside functions at lines {inner}"
