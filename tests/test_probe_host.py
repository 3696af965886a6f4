"""Host-side contract of latent classification (TorchMMVAE.latents_for / classify_latents, csrc/probe.hip): the C-ABI
exports are declared, bound and built; argument errors are raised before any kernel runs (the models live on the CPU
here, where no kernel can run); the probe table's order; the seeded init.  Numerics: test_probe_gpu.py."""
import ctypes
import math
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


def _batch(B=4, T=6, seed=3):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    return cdsprites_batch(B, T, seed=seed)


def _sets(labels=None, B=4):
    y = torch.arange(B) % 3 if labels is None else labels
    return [(_batch(B), y)], [(_batch(B, seed=4), y)]


def test_exports_are_declared_bound_and_built():
    from multimodal_vae_comparison_amd import hipops
    lib = ctypes.CDLL(hipops.LIB_PATH)
    header = open(f"{ROOT}/include/mmvae_hip.h").read()
    for name in ("mmvae_probe_train", "mmvae_probe_eval", "mmvae_probe_tile_rows"):
        assert name in hipops.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert hipops.PROBE_MAX_CLASSES == int(re.search(r"#define MMVAE_PROBE_MAX_CLASSES (\d+)", header).group(1)) == 32
    assert hipops.PROBE_MAX_PROBES == int(re.search(r"#define MMVAE_PROBE_MAX_PROBES (\d+)", header).group(1))
    makefile = open(f"{ROOT}/multimodal_vae_comparison_amd/csrc/Makefile").read()
    assert "probe.hip" in makefile


def test_no_new_environment_knob():
    for f in ("multimodal_vae_comparison_amd/csrc/probe.hip",):
        assert "getenv" not in open(f"{ROOT}/{f}").read()


@pytest.mark.parametrize("mixing", ["poe", "moe", "mopoe"])
def test_training_mode_is_refused(mixing):
    tr = _trainer(mixing)
    tr.model.train()
    with pytest.raises(RuntimeError, match="eval"):
        tr.model.latents_for(_batch(), ["mod_1"])
    train, test = _sets()
    with pytest.raises(RuntimeError, match="eval"):
        tr.model.classify_latents(train, test, 3)
    with pytest.raises(RuntimeError, match="eval"):
        tr.classify_latents(train, test, 3)


def test_label_outside_the_class_count_is_refused():
    tr = _trainer("mopoe")
    train, test = _sets(torch.tensor([0, 1, 2, 3]))
    with pytest.raises(ValueError, match="labels"):
        tr.model.classify_latents(train, test, 3)
    train, test = _sets(torch.tensor([0, 1, -1, 2]))
    with pytest.raises(ValueError, match="labels"):
        tr.model.classify_latents(train, test, 3)
    # one bad column of two
    y = torch.tensor([[0, 0], [1, 1], [2, 5], [0, 1]])
    train, test = _sets(y)
    with pytest.raises(ValueError, match="column 1"):
        tr.model.classify_latents(train, test, [3, 5])


@pytest.mark.parametrize("C", [1, 33, 0])
def test_class_count_outside_2_to_32_is_refused(C):
    tr = _trainer("mopoe")
    train, test = _sets(torch.zeros(4, dtype=torch.long))
    with pytest.raises(ValueError, match="classes"):
        tr.model.classify_latents(train, test, C)
    from multimodal_vae_comparison_amd import ops
    with pytest.raises(ValueError, match="classes"):
        ops.probe_state(1, 8, C, "cpu")


def test_more_than_256_latent_dimensions_are_refused():
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.synthetic import MS_MODS, mnist_svhn_batch
    tr = _trainer("mopoe", MS_MODS, D=257)      # (the MNIST / SVHN towers build at any width)
    y = torch.arange(4) % 3
    train, test = [(mnist_svhn_batch(4, seed=1), y)], [(mnist_svhn_batch(4, seed=2), y)]
    with pytest.raises(ValueError, match="257"):
        tr.model.classify_latents(train, test, 3)
    with pytest.raises(ValueError, match="257"):
        ops.probe_state(1, 257, 3, "cpu")


def test_given_must_name_modalities_with_data():
    tr = _trainer("moe")
    b = _batch()
    b["mod_2"] = dict(b["mod_2"], data=None)
    with pytest.raises(ValueError, match="data"):
        tr.model.latents_for(b, ["mod_2"])
    with pytest.raises(ValueError, match="data"):
        tr.model.latents_for(b, ["mod_1", "mod_2"])
    with pytest.raises(ValueError, match="data"):
        tr.model.latents_for(b, [])
    y = torch.arange(4) % 3
    with pytest.raises(ValueError, match="data"):
        tr.model.classify_latents([(b, y)], [(b, y)], 3)      # the default `given` holds mod_2
    with pytest.raises(ValueError, match="modalities of this model"):
        tr.model.classify_latents([(_batch(), y)], [(_batch(), y)], 3, given=[["mod_9"]])
    with pytest.raises(ValueError, match="not a modality"):
        tr.model.latents_for(_batch(), ["mod_1"], of="mod_9")


def test_unimodal_vae_refuses_by_name():
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    uni = _trainer("mopoe", [CD_MODS[0]])
    assert type(uni.model).__name__ == "VAE"
    with pytest.raises(NotImplementedError, match="unimodal"):
        uni.model.latents_for({}, ["mod_1"])
    with pytest.raises(NotImplementedError, match="unimodal"):
        uni.classify_latents([], [], 3)


def test_probe_table_order():
    """default `given` = every single modality, then all together; probe p = s * A + a"""
    m = _trainer("mopoe").model
    y = torch.zeros(4, 2, dtype=torch.long)
    given, keys, probes = m.probe_table([3, 5], y.shape[1])
    assert given == [["mod_1"], ["mod_2"], ["mod_1", "mod_2"]]
    assert keys == ["mod_1", "mod_2", "mod_1+mod_2"]
    assert probes == [(0, 0, 3), (0, 1, 5), (1, 0, 3), (1, 1, 5), (2, 0, 3), (2, 1, 5)]
    assert len(probes) == len(given) * y.shape[1]
    # an int serves every column; names are put in modality order
    given, keys, probes = m.probe_table(4, 2, given=[["mod_2", "mod_1"]])
    assert keys == ["mod_1+mod_2"] and probes == [(0, 0, 4), (0, 1, 4)]
    with pytest.raises(ValueError, match="class counts"):
        m.probe_table([3], 2)


def test_seeded_init_is_reproducible_and_inside_the_linear_bound():
    from multimodal_vae_comparison_amd import ops
    P, D, C = 4, 20, 10
    a, b, c = ops.probe_state(P, D, C, "cpu", seed=5), ops.probe_state(P, D, C, "cpu", seed=5), ops.probe_state(P, D, C, "cpu", seed=6)
    assert a.shape == (P, 3, C, D + 1) and a.dtype == torch.float32
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert float(a[:, 0].abs().max()) <= 1.0 / math.sqrt(D)
    assert float(a[:, 0].abs().max()) > 0.9 / math.sqrt(D), "uniform over the whole interval"
    assert float(a[:, 1:].abs().max()) == 0.0, "the moments start at zero"
    W, bias = ops.probe_weights(a, 2, 7)
    assert W.shape == (7, D) and bias.shape == (7,)
    assert torch.equal(W, a[2, 0, :7, :D]) and torch.equal(bias, a[2, 0, :7, D])
    # given weights: rows beyond C stay zero
    Wi, bi = torch.randn(3, D), torch.randn(3)
    s = ops.probe_state(1, D, C, "cpu", init=[(Wi, bi)])
    W2, b2 = ops.probe_weights(s, 0, 3)
    assert torch.equal(W2, Wi) and torch.equal(b2, bi) and float(s[0, 0, 3:].abs().max()) == 0.0


def test_wrappers_refuse_bad_arguments_before_any_launch():
    """CPU tensors here: reaching a launch would raise the binding's AssertionError instead"""
    from multimodal_vae_comparison_amd import ops
    N, D = 12, 8
    st = ops.probe_state(1, D, 4, "cpu")
    z = torch.zeros(1, N, D)
    y = (torch.arange(N, dtype=torch.int32) % 5).reshape(1, N)      # label 4 >= C = 4
    with pytest.raises(ValueError, match="labels"):
        ops.probe_train(st, z, y, [(0, 0, 4)], 4, 0, 3)
    with pytest.raises(ValueError, match="classes"):
        ops.probe_train(st, z, y, [(0, 0, 5)], 4, 0, 3)             # C > Cmax of the state
    with pytest.raises(ValueError, match="batch"):
        ops.probe_train(st, z, y % 4, [(0, 0, 4)], 0, 0, 3)
    with pytest.raises(ValueError, match="outside"):
        ops.probe_train(st, z, y % 4, [(1, 0, 4)], 4, 0, 3)
    with pytest.raises(AssertionError):
        ops.probe_train(st, z, y % 4, [(0, 0, 4)], 4, 0, 3)         # valid: only the device is missing


def test_tile_rows_table():
    """rows of a latent tile per D: the largest power of two <= 256 with 32 (D + 1) + rows ((D + 1 | 1) + 33) + 8 floats
    inside 64 KB of LDS and rows D <= 8192 prefetched elements"""
    from multimodal_vae_comparison_amd import hipops
    lib = ctypes.CDLL(hipops.LIB_PATH)
    for D in range(1, 257):
        want = 256
        while want > 16 and (want * D > 8192 or 32 * (D + 1) + want * (((D + 1) | 1) + 33) + 8 > 16384):
            want //= 2
        assert lib.mmvae_probe_tile_rows(D) == want, D
        assert 32 * (D + 1) + want * (((D + 1) | 1) + 33) + 8 <= 16384 and want * D <= 8192
    got = {D: lib.mmvae_probe_tile_rows(D) for D in (16, 20, 26, 27, 32, 64, 65, 128, 256)}
    assert got == {16: 256, 20: 256, 26: 256, 27: 128, 32: 128, 64: 128, 65: 64, 128: 64, 256: 16}, got
    assert lib.mmvae_probe_tile_rows(0) == 0 and lib.mmvae_probe_tile_rows(257) == 0


def test_more_probes_than_one_launch_takes_are_refused():
    from multimodal_vae_comparison_amd import hipops
    tr = _trainer("mopoe")
    A = hipops.PROBE_MAX_PROBES // 3 + 1      # 3 subsets x A columns > 64
    y = torch.zeros(4, A, dtype=torch.long)
    with pytest.raises(ValueError, match="probes"):
        tr.model.classify_latents([(_batch(), y)], [(_batch(), y)], 2)
