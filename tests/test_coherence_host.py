"""Host-side contract of generation coherence (multimodal_vae_comparison_amd/coherence.py, TorchMMVAE.cross_coherence /
joint_coherence, csrc/coherence.hip): the caption semantics reproduce every case recorded from the reference
(tests/golden/coherence/text_cases.json); the classifier module takes the reference's state-dict keys; the C-ABI exports
are declared, bound and built; argument and mode errors are raised before any kernel runs (the models live on the CPU
here).  Numerics: test_coherence_gpu.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

COH_DIR = os.path.join(GOLDEN_DIR, "coherence")


def _text_fixture():
    with open(os.path.join(COH_DIR, "text_cases.json")) as f:
        return json.load(f)


TEXT = _text_fixture()
CASE_IDS = [f"{i}-L{c['level']}-{c['what'][:28].replace(' ', '_')}" for i, c in enumerate(TEXT["cases"])]


def load_fixture_classifier(att):
    """the fixture's reference CNN parameters (fp16 on disk) as a state dict, lin2 zero-filled"""
    z = np.load(os.path.join(COH_DIR, f"classifier_{att}.npz"))
    sd = {k: torch.from_numpy(z[k].astype(np.float32)) for k in z.files}
    sd["lin2.module.weight"] = torch.zeros(256, 256)
    sd["lin2.module.bias"] = torch.zeros(256)
    return sd


def _trainer(mixing, D=8, private=None):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    mods = [dict(m, private=private) for m in CD_MODS] if private else CD_MODS
    cfg, dims = config_from_mods(mixing, mods, D, batch_size=4)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cpu")
    tr.model.eval()
    return tr


def _batch(B=4, T=6, seed=3):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    return cdsprites_batch(B, T, seed=seed)


# ---- text semantics ---------------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_should():
    cases = TEXT["cases"]
    assert len(cases) >= 60
    assert {c["level"] for c in cases} == {1, 2, 3, 4, 5}
    assert any(c["caption"] == c["decoded"] for c in cases)
    assert any(len(c["decoded"]) < len(c["caption"]) for c in cases)
    assert any(len(c["decoded"]) > len(c["caption"]) for c in cases)
    assert any(c["decoded"].endswith("  ") for c in cases)
    assert any("Unknown" in c["retrieved"] for c in cases)
    assert any(c["strict"] == 1 for c in cases) and any(c["strict"] == 0 for c in cases)
    # strict is "every letter right", not "every attribute right": some case has all features and is not strict
    assert any(c["features"] == 1.0 and c["strict"] == 0 for c in cases)


def test_tables_match_the_reference():
    from multimodal_vae_comparison_amd import coherence as coh
    t = TEXT["tables"]
    assert {int(k): tuple(v) for k, v in t["level_attributes"].items()} == coh.LEVEL_ATTRIBUTES
    assert {k: tuple(v) for k, v in t["class_mappings"].items()} == coh.CLASS_NAMES


@pytest.mark.parametrize("case", TEXT["cases"], ids=CASE_IDS)
def test_text_restatement_reproduces_the_reference(case):
    from multimodal_vae_comparison_amd import coherence as coh
    level, caption, decoded = case["level"], case["caption"], case["decoded"]
    strict, feats, letters = coh.score_decoded_text(level, caption, decoded)
    assert (strict, feats, letters) == (case["strict"], case["features"], case["letters"])
    assert coh.retrieve_attributes(decoded, level) == case["retrieved"]
    for a in coh.LEVEL_ATTRIBUTES[level]:
        assert coh.attribute_in_caption(a, caption) == case["caption_attributes"][a]
        assert coh.attribute_in_caption(a, case["retrieved"]) == case["retrieved_attributes"][a]
    # the same through token ids, as the device path hands them over (padding decodes to spaces)
    T = max(len(caption), len(decoded)) + 3
    cap_ids, dec_ids = coh.text_to_ids(caption, T), coh.text_to_ids(decoded, T)
    assert coh.ids_to_text(cap_ids, len(caption)) == caption
    assert coh.ids_to_text(dec_ids, len(decoded)) == decoded
    same = sum(1 for t in range(min(len(caption), T)) if cap_ids[t] == dec_ids[t])
    # a decoded string padded with spaces to T agrees with the caption wherever the unpadded one does, plus at the
    # caption's own spaces beyond the decoded string's end
    padded = coh.ids_to_text(dec_ids)
    assert same == coh.count_same_letters(padded, caption)
    labels = coh.caption_labels(level, caption)
    for a, y in zip(coh.LEVEL_ATTRIBUTES[level], labels):
        v = case["caption_attributes"][a]
        assert y == (coh.CLASS_NAMES[a].index(v) if v in coh.CLASS_NAMES[a] else -1)


def test_unknown_never_matches_and_white_has_no_class():
    from multimodal_vae_comparison_amd import coherence as coh
    assert coh.caption_labels(3, "Unknown Unknown Unknown") == [-1, -1, -1]
    assert coh.caption_labels(3, "big white heart") == [0, -1, 2]
    with pytest.raises(ValueError, match="level"):
        coh.retrieve_attributes("big heart", 6)


# ---- classifiers ------------------------------------------------------------------------------------------------------
REFERENCE_KEYS = [f"{layer}.module.{p}" for layer in ("conv1", "conv2", "conv3", "conv_64", "lin1", "lin2", "fc")
                  for p in ("weight", "bias")]


@pytest.mark.parametrize("C", [2, 3, 5])
def test_classifier_takes_the_reference_state_dict(C):
    from multimodal_vae_comparison_amd.coherence import AttributeClassifier
    net = AttributeClassifier(C)
    assert sorted(net.state_dict().keys()) == sorted(REFERENCE_KEYS)
    shapes = {"conv1.module.weight": (32, 3, 4, 4), "conv2.module.weight": (32, 32, 4, 4),
              "conv3.module.weight": (32, 32, 4, 4), "conv_64.module.weight": (32, 32, 4, 4),
              "lin1.module.weight": (256, 512), "lin2.module.weight": (256, 256), "fc.module.weight": (C, 256)}
    g = torch.Generator().manual_seed(C)
    sd = {}
    for k in REFERENCE_KEYS:
        shape = shapes[k] if k.endswith("weight") else (shapes[k.replace("bias", "weight")][0],)
        sd[k] = torch.randn(*shape, generator=g)
    assert net.load_state_dict(sd, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k])
    assert not any(p.requires_grad for p in net.parameters())


@pytest.mark.parametrize("att,C", [("shape", 3), ("color", 5)])
def test_fixture_classifier_loads_strictly(att, C):
    from multimodal_vae_comparison_amd.coherence import AttributeClassifier
    sd = load_fixture_classifier(att)
    net = AttributeClassifier(C)
    net.load_state_dict(sd, strict=True)
    # fp16-representable: both sides compute with identical fp32 values
    for k, v in sd.items():
        assert torch.equal(v, v.half().float()), k
    with pytest.raises(RuntimeError):
        AttributeClassifier(C + 1).load_state_dict(sd, strict=True)


@pytest.mark.parametrize("C", [1, 9, 0])
def test_classifier_class_count_outside_2_to_8_is_refused(C):
    from multimodal_vae_comparison_amd.coherence import AttributeClassifier
    with pytest.raises(ValueError, match="classes"):
        AttributeClassifier(C)


def test_classifier_sets_are_checked():
    from multimodal_vae_comparison_amd import coherence as coh
    with pytest.raises(ValueError, match="classifiers"):
        coh.AttributeClassifiers({})
    with pytest.raises(TypeError):
        coh.AttributeClassifiers({"shape": torch.nn.Linear(2, 2)})
    cls = coh.AttributeClassifiers.for_level(5)
    assert cls.attributes == list(coh.LEVEL_ATTRIBUTES[5]) and cls.n_classes == [2, 5, 3, 4, 2]
    assert coh.check_classifiers(cls, 5) is cls
    assert coh.check_classifiers(cls, 2).attributes == ["size", "shape"]
    with pytest.raises(ValueError, match="missing"):
        coh.check_classifiers(coh.AttributeClassifiers.for_level(2), 3)
    with pytest.raises(ValueError, match="classes"):
        coh.check_classifiers(coh.AttributeClassifiers({"shape": coh.AttributeClassifier(4)}), 1)
    with pytest.raises(TypeError):
        coh.check_classifiers({"shape": coh.AttributeClassifier(3)}, 1)


def test_quantisation_is_the_uint8_round_trip():
    from multimodal_vae_comparison_amd.coherence import quantise_images
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 1, 3, 64, 64, generator=g)
    x.view(-1)[:4] = torch.tensor([0.0, 1.0, 0.999999, 1.0 / 255])
    ref = torch.from_numpy((np.asarray(x) * 255).astype(np.uint8).reshape(-1, 3, 64, 64)) / 255
    assert torch.equal(quantise_images(x), ref)
    k = torch.arange(256, dtype=torch.float32) / 255      # an 8-bit image survives it unchanged
    assert torch.equal(quantise_images(k.repeat(48)[:12288].reshape(1, 3, 64, 64)).view(-1)[:256], k)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_bound_and_built():
    from multimodal_vae_comparison_amd import hipops
    lib = ctypes.CDLL(hipops.LIB_PATH)
    header = open(f"{ROOT}/include/mmvae_hip.h").read()
    for name in ("mmvae_text_decode_score", "mmvae_cls_head"):
        assert name in hipops.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    for py, c in (("COH_MAX_STEPS", "MMVAE_COH_MAX_STEPS"), ("COH_MAX_VOCAB", "MMVAE_COH_MAX_VOCAB"),
                  ("COH_MAX_CLASSIFIERS", "MMVAE_COH_MAX_CLASSIFIERS"), ("COH_MAX_CLASSES", "MMVAE_COH_MAX_CLASSES"),
                  ("COH_FEATS", "MMVAE_COH_FEATS"), ("COH_HIDDEN", "MMVAE_COH_HIDDEN")):
        assert getattr(hipops, py) == int(re.search(rf"#define {c} (\d+)", header).group(1))
    assert "coherence.hip" in open(f"{ROOT}/multimodal_vae_comparison_amd/csrc/Makefile").read()
    assert "getenv" not in open(f"{ROOT}/multimodal_vae_comparison_amd/csrc/coherence.hip").read()


def test_kernels_refuse_shapes_outside_their_bounds():
    """the C entry points return their error codes before any launch (null pointers never reach a kernel)"""
    from multimodal_vae_comparison_amd import hipops
    L = hipops.lib()
    one = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: every call below is refused first
    assert L.mmvae_text_decode_score(None, None, None, one, None, 1, 4, 4, None) == 1
    assert L.mmvae_text_decode_score(one, one, None, one, None, 1, 4, 4, None) == 1
    for T, V in ((0, 27), (257, 27), (9, 1), (9, 257)):
        assert L.mmvae_text_decode_score(one, None, None, one, None, 1, T, V, None) == 2
    nc = (ctypes.c_int * 9)(*([3] * 9))
    assert L.mmvae_cls_head(None, one, one, one, one, nc, None, one, None, None, None, 1, 1, 3, None) == 1
    assert L.mmvae_cls_head(one, one, one, one, one, nc, one, one, None, None, None, 1, 1, 3, None) == 1
    assert L.mmvae_cls_head(one, one, one, one, one, nc, None, one, None, None, None, 9, 1, 3, None) == 2
    assert L.mmvae_cls_head(one, one, one, one, one, nc, None, one, None, None, None, 1, 1, 9, None) == 2
    assert L.mmvae_cls_head(one, one, one, one, one, nc, None, one, None, None, None, 1, 1, 2, None) == 2      # C 3 > Cmax 2
    nc[0] = 1
    assert L.mmvae_cls_head(one, one, one, one, one, nc, None, one, None, None, None, 1, 1, 3, None) == 2


def test_ops_wrappers_check_their_arguments():
    from multimodal_vae_comparison_amd import ops
    with pytest.raises(ValueError, match="T = 300"):
        ops.text_decode_score(torch.zeros(1, 300, 27))
    with pytest.raises(ValueError, match="V = 1"):
        ops.text_decode_score(torch.zeros(1, 3, 1))
    with pytest.raises(ValueError, match="together"):
        ops.text_decode_score(torch.zeros(1, 3, 4), target_ids=torch.zeros(1, 3, dtype=torch.int32))
    f, W1, b1 = torch.zeros(1, 2, 512), torch.zeros(1, 256, 512), torch.zeros(1, 256)
    with pytest.raises(ValueError, match="class counts"):
        ops.cls_head(f, W1, b1, torch.zeros(1, 9, 256), torch.zeros(1, 9), [3])
    with pytest.raises(ValueError, match="class counts"):
        ops.cls_head(f, W1, b1, torch.zeros(1, 3, 256), torch.zeros(1, 3), [4])
    with pytest.raises(ValueError, match="classifiers"):
        ops.cls_head(f, W1, b1, torch.zeros(1, 3, 256), torch.zeros(1, 3), [3, 3])


# ---- the public methods -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixing", ["poe", "moe", "mopoe"])
def test_training_mode_is_refused(mixing):
    from multimodal_vae_comparison_amd.coherence import AttributeClassifiers
    tr = _trainer(mixing)
    cls = AttributeClassifiers.for_level(3)
    tr.model.train()
    with pytest.raises(RuntimeError, match="eval"):
        tr.model.cross_coherence([_batch()], cls, 3)
    with pytest.raises(RuntimeError, match="eval"):
        tr.model.joint_coherence(cls, 3, n=4)
    with pytest.raises(RuntimeError, match="eval"):
        tr.cross_coherence([_batch()], cls, 3)
    with pytest.raises(RuntimeError, match="eval"):
        tr.joint_coherence(cls, 3, n=4)


def test_arguments_are_checked_before_anything_runs():
    from multimodal_vae_comparison_amd.coherence import AttributeClassifiers
    tr = _trainer("mopoe")
    cls = AttributeClassifiers.for_level(3)
    with pytest.raises(ValueError, match="level"):
        tr.model.cross_coherence([_batch()], cls, 7)
    with pytest.raises(ValueError, match="missing"):
        tr.model.cross_coherence([_batch()], AttributeClassifiers.for_level(2), 3)
    with pytest.raises(TypeError):
        tr.model.joint_coherence({"shape": None}, 1)
    with pytest.raises(ValueError, match="modalities"):
        tr.model.cross_coherence([_batch()], cls, 3, image="mod_1", text="mod_9")
    with pytest.raises(ValueError, match="modalities"):
        tr.model.joint_coherence(cls, 3, image="mod_1", text="mod_1")
    with pytest.raises(ValueError, match="n = 0"):
        tr.model.joint_coherence(cls, 3, n=0)
    with pytest.raises(ValueError, match="empty"):
        tr.model.cross_coherence([], cls, 3)
    b = _batch()
    b["mod_1"] = dict(b["mod_1"], data=None)
    with pytest.raises(ValueError, match="every batch"):
        tr.model.cross_coherence([b], cls, 3)
    assert tr.model._eval_draws is False and tr.model.eps_override is None


def test_private_latents_have_no_joint_sample():
    from multimodal_vae_comparison_amd.coherence import AttributeClassifiers
    tr = _trainer("dmvae", private=4)
    with pytest.raises(NotImplementedError, match="private"):
        tr.model.joint_coherence(AttributeClassifiers.for_level(1), 1)


def test_unimodal_vae_refuses_by_name():
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods("mopoe", CD_MODS[:1], 8, batch_size=4)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cpu")
    with pytest.raises(NotImplementedError, match="cross_coherence"):
        tr.model.cross_coherence([], None, 1)
    with pytest.raises(NotImplementedError, match="joint_coherence"):
        tr.model.joint_coherence(None, 1)
