"""Host-side contract of the held-out log-likelihood estimator (TorchMMVAE.estimate_log_likelihood): argument errors are
raised before any kernel runs, the default chunk rule, and the new C-ABI exports are declared, bound and built.  Models
live on the CPU here (no GPU); the numerics are checked on the GPU in test_loglik_gpu.py."""
import ctypes
import re

import pytest
import torch

from conftest import ROOT


def _trainer(mixing, mods=None, D=8, **extra):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, mods or CD_MODS, D, batch_size=4, **extra)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cpu")
    tr.model.eval()
    return tr


def _batch(B=4, T=6):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    return cdsprites_batch(B, T, seed=3)


@pytest.mark.parametrize("mixing,K", [("moe", 3), ("mopoe", 4), ("mopoe", 7), ("poe", 0)])
def test_k_must_be_a_multiple_of_the_components(mixing, K):
    """C = 2 (moe) / 3 (mopoe) / 1 (poe) for two given modalities: stratified draws need K % C == 0, K >= 1"""
    tr = _trainer(mixing)
    with pytest.raises(ValueError, match="multiple"):
        tr.model.estimate_log_likelihood(_batch(), K)
    with pytest.raises(ValueError, match="multiple"):
        tr.estimate_log_likelihood(_batch(), K)


def test_single_given_modality_changes_the_component_count(monkeypatch):
    """given = one modality: C = 1 for every mixer, so K = 4 passes mopoe's multiple check and the estimator goes on to
    build the proposal (replaced here by a sentinel: the towers need the GPU)"""
    tr = _trainer("mopoe")

    class Reached(Exception):
        pass

    def proposal(mods, given):
        raise Reached(tuple(given))

    monkeypatch.setattr(tr.model, "_proposal", proposal)
    with pytest.raises(ValueError, match="multiple"):
        tr.model.estimate_log_likelihood(_batch(), 4, given=["mod_1", "mod_2"])
    with pytest.raises(Reached) as e:
        tr.model.estimate_log_likelihood(_batch(), 4, given=["mod_1"])
    assert e.value.args[0] == ("mod_1",)


def test_dmvae_and_unimodal_have_no_joint_proposal():
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, MS_MODS
    tr = _trainer("dmvae", [dict(m, private=4) for m in MS_MODS])
    with pytest.raises(NotImplementedError, match="dmvae"):
        tr.model.estimate_log_likelihood({}, 4)
    tr.model.train()      # the mixer is named whatever the mode
    with pytest.raises(NotImplementedError, match="dmvae"):
        tr.estimate_log_likelihood({}, 4)
    uni = _trainer("mopoe", [CD_MODS[0]])
    assert type(uni.model).__name__ == "VAE"
    with pytest.raises(NotImplementedError, match="unimodal"):
        uni.estimate_log_likelihood({}, 4)


@pytest.mark.parametrize("mixing", ["poe", "moe", "mopoe"])
def test_training_mode_is_refused(mixing):
    tr = _trainer(mixing)
    tr.model.train()
    with pytest.raises(RuntimeError, match="eval"):
        tr.model.estimate_log_likelihood(_batch(), 6)


def test_given_and_targets_need_data():
    tr = _trainer("moe")
    b = _batch()
    b["mod_2"] = dict(b["mod_2"], data=None)
    with pytest.raises(ValueError, match="data"):
        tr.model.estimate_log_likelihood(b, 4, given=["mod_1"], targets=["mod_2"])
    with pytest.raises(ValueError, match="data"):
        tr.model.estimate_log_likelihood(b, 4, given=[])


@pytest.mark.parametrize("K,C,B,want", [
    (512, 1, 128, 8),        # 8 * 128 = 1024 rows
    (510, 3, 128, 6),        # multiples of 3 dividing 510 with <= 8 samples: 3, 6
    (1000, 2, 64, 10),       # <= 16 samples: 2, 4, 8, 10
    (12, 3, 2000, 3),        # nothing fits 1024 rows: at least C
    (7, 7, 1, 7),
    (30, 1, 1, 30),          # K itself when it fits
    (2048, 1, 1, 1024),
    (14, 7, 100, 7),
])
def test_default_k_chunk(K, C, B, want):
    from multimodal_vae_comparison_amd.models.mmvae_base import TorchMMVAE
    kc = TorchMMVAE.default_k_chunk(K, C, B)
    assert kc == want
    assert kc % C == 0 and K % kc == 0 and (kc * B <= 1024 or kc == C)


def test_proposal_sizes():
    for mixing, sizes in (("poe", (1, 1, 1)), ("moe", (1, 2, 3)), ("mopoe", (1, 3, 7))):
        m = _trainer(mixing).model
        assert tuple(m._proposal_size(n) for n in (1, 2, 3)) == sizes


def test_evaluation_has_its_own_generator_state():
    m = _trainer("mopoe").model
    assert m._eval_rng_state.data_ptr() != m._rng_state.data_ptr()
    assert "_eval_rng_state" not in m.state_dict()
    assert int(m._eval_rng_state[0]) != int(m._rng_state[0]), "a stream of its own, not a copy of the training stream"


def test_new_exports_are_declared_bound_and_built():
    from multimodal_vae_comparison_amd import hipops
    lib = ctypes.CDLL(hipops.LIB_PATH)
    header = open(f"{ROOT}/include/mmvae_hip.h").read()
    for name in ("mmvae_mix_ksample_logw_fwd", "mmvae_lme_update", "mmvae_lme_finish"):
        assert name in hipops.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert hipops.MIX_MAX_COMPONENTS == int(re.search(r"#define MMVAE_MIX_MAX_COMPONENTS (\d+)", header).group(1))
    makefile = open(f"{ROOT}/multimodal_vae_comparison_amd/csrc/Makefile").read()
    assert "loglik.hip" in makefile


def test_wrappers_refuse_cpu_tensors():
    """no fallback: the ops need device memory"""
    from multimodal_vae_comparison_amd import ops
    comps = torch.zeros(1, 2, 8)
    with pytest.raises(AssertionError):
        ops.mix_ksample_logw(comps, [False], torch.zeros(1, 4), 2, eps=torch.zeros(2, 2, 4))
