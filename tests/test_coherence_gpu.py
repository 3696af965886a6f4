"""Generation coherence on the GPU (csrc/coherence.hip, multimodal_vae_comparison_amd/coherence.py,
TorchMMVAE.cross_coherence / joint_coherence).

  text_decode_score   against torch.argmax and a Python count: exact.
  cls_head            against an fp64 computation.  The logits are held to twice the fp32 rounding bound of the two
                      dot products, evaluated in fp64 per element:
                          bound = 2 (g(514) |W2| (|W1| relu(x) + |b1|) + g(258) (|W2| h + |b2|)),  g(n) = n u / (1 - n u),
                      u = 2^-24 (a 512-term sum, its bias and the ReLU-free pass through the second layer; a 256-term sum
                      and its bias).  pred must equal the fp64 argmax on every row whose fp64 top-two margin exceeds
                      twice that bound; at most 2 % of the rows may fall inside it (the inputs are seeded so that the fp64
                      computation alone stays under the cap: checked without a GPU below).
  fixture classifiers the reference's names and fp64 logits for 12 images; the four convs add their error to the head's,
                      so the logits are held to the tolerance the Enc_CNN2 tower is held to against the oracle
                      (max |a - b| <= 1e-5 max |b|, tests/test_oracle_golden.py).
  end to end          MoPoE and PoE at B = 6, T = 9, D = 8 against a recomputation from forward()'s own decoder outputs.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_coherence_host import COH_DIR, load_fixture_classifier

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- text_decode_score --------------------------------------------------------------------------------------------------
def _text_inputs(N, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, T, V, generator=g)
    # a third of the rows on a coarse grid: equal maxima are common there, the first index must win
    coarse = torch.randint(0, 3, (N, T, V), generator=g).float()
    pick = torch.rand(N, T, generator=g)
    logits = torch.where((pick < 0.33)[..., None], coarse, logits)
    logits = torch.where(((pick >= 0.33) & (pick < 0.5))[..., None], torch.zeros(()), logits)      # all-zero rows (padding)
    logits[0, 0] = 0.0
    logits[-1, -1] = 1.0      # every entry the maximum
    target = torch.randint(0, V, (N, T), generator=g, dtype=torch.int32)
    ref_pred = torch.argmax(logits, dim=-1)
    agree = torch.rand(N, T, generator=g) < 0.5
    target = torch.where(agree, ref_pred.int(), target)
    lengths = torch.randint(0, T + 4, (N,), generator=g, dtype=torch.int32)      # 0 and more than T included
    lengths[0] = 0
    lengths[-1] = T + 3
    return logits, target, lengths, ref_pred


@pytest.mark.gpu
@pytest.mark.parametrize("V", [2, 27, 64, 65])
@pytest.mark.parametrize("T", [1, 7, 64, 65])
@pytest.mark.parametrize("N", [1, 3, 130])
def test_text_decode_score_is_exact(hip_lib, N, T, V):
    from multimodal_vae_comparison_amd import ops
    logits, target, lengths, ref_pred = _text_inputs(N, T, V, seed=1000 * N + 10 * T + V)
    lp, tp, ln = ref_pred.tolist(), target.tolist(), lengths.tolist()
    ref_letters = [sum(1 for t in range(min(ln[n], T)) if lp[n][t] == tp[n][t]) for n in range(N)]
    pred, letters = ops.text_decode_score(logits.cuda(), target.cuda(), lengths.cuda())
    assert pred.dtype == torch.int32 and letters.dtype == torch.int32
    assert torch.equal(pred.cpu().long(), ref_pred)
    assert letters.cpu().tolist() == ref_letters
    assert bool((pred[0, 0] == 0).item())
    # null targets: only pred
    pred2, none = ops.text_decode_score(logits.cuda())
    assert none is None and torch.equal(pred2, pred)


# ---- cls_head -----------------------------------------------------------------------------------------------------------
CLASS_MIX = [3, 2, 5, 3, 2]
CMAX = 5


def _head_inputs(N, A, seed):
    g = torch.Generator().manual_seed(seed)
    C = CLASS_MIX[:A]
    # a conv output before its ReLU, mostly negative: the ReLU leaves a sparse input, as a trained trunk does, and the
    # rounding bound (which grows with sum |W1| relu(x)) stays small against the logits' margins
    feats = torch.randn(A, N, 512, generator=g) - 1.0
    k1, k2 = 1.0 / math.sqrt(512.0), 1.0 / math.sqrt(256.0)
    W1 = (torch.rand(A, 256, 512, generator=g) * 2 - 1) * k1
    b1 = (torch.rand(A, 256, generator=g) * 2 - 1) * k1
    W2 = (torch.rand(A, CMAX, 256, generator=g) * 2 - 1) * k2
    b2 = (torch.rand(A, CMAX, generator=g) * 2 - 1) * 2.0 * k2
    labels = torch.stack([torch.randint(-1, c, (N,), generator=g, dtype=torch.int32) for c in C])      # some are -1
    labels[0, 0] = -1
    return feats, W1, b1, W2, b2, C, labels


def _head_fp64(feats, W1, b1, W2, b2, C):
    """-> per classifier (logits (N,C), bound (N,C)) in fp64"""
    out = []
    for a, c in enumerate(C):
        x = feats[a].double().clamp_min(0)
        w1, bb1, w2, bb2 = W1[a].double(), b1[a].double(), W2[a, :c].double(), b2[a, :c].double()
        h = (x @ w1.t() + bb1).clamp_min(0)
        logits = h @ w2.t() + bb2
        herr = x @ w1.abs().t() + bb1.abs()
        bound = 2.0 * (gamma(514) * (herr @ w2.abs().t()) + gamma(258) * (h @ w2.abs().t() + bb2.abs()))
        out.append((logits, bound))
    return out


def _decided(logits, bound):
    """rows whose fp64 top-two margin exceeds twice the (largest) bound of the row"""
    top = logits.topk(2, dim=-1).values
    return (top[:, 0] - top[:, 1]) > 2.0 * bound.max(-1).values


HEAD_SHAPES = [(N, A) for N in (1, 63, 64, 65, 257) for A in (1, 5)]


@pytest.mark.parametrize("N,A", HEAD_SHAPES)
def test_cls_head_inputs_stay_under_the_skip_cap(N, A):
    """the fp64 computation alone: at most 2 % of the rows have a top-two margin inside twice the bound"""
    feats, W1, b1, W2, b2, C, _ = _head_inputs(N, A, seed=7 * N + A)
    ref = _head_fp64(feats, W1, b1, W2, b2, C)
    skipped = sum(int((~_decided(l, b)).sum()) for l, b in ref)
    assert skipped <= 0.02 * N * A, (skipped, N * A)


@pytest.mark.gpu
@pytest.mark.parametrize("N,A", HEAD_SHAPES)
def test_cls_head_against_fp64(hip_lib, N, A):
    from multimodal_vae_comparison_amd import ops
    feats, W1, b1, W2, b2, C, labels = _head_inputs(N, A, seed=7 * N + A)
    ref = _head_fp64(feats, W1, b1, W2, b2, C)
    out = ops.cls_head(feats.cuda(), W1.cuda(), b1.cuda(), W2.cuda(), b2.cuda(), C, labels=labels.cuda(), want_logits=True)
    pred, logits = out["pred"].cpu().long(), out["logits"].cpu().double()
    correct, n_correct = out["correct"].cpu(), out["n_correct"].cpu()
    skipped, worst = 0, 0.0
    for a, c in enumerate(C):
        l64, bound = ref[a]
        err = (logits[a, :, :c] - l64).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), f"classifier {a}: logit error {float((err / bound).max()):.3f} x the bound"
        assert bool((logits[a, :, c:] == 0).all())
        ok = _decided(l64, bound)
        skipped += int((~ok).sum())
        assert torch.equal(pred[a][ok], l64.argmax(-1)[ok])
        assert bool(((pred[a] >= 0) & (pred[a] < c)).all())
        # the device's own argmax is the first maximum of the device's own logits
        assert torch.equal(pred[a], logits[a, :, :c].argmax(-1))
    print(f"cls_head N {N} A {A}: worst logit error {worst:.4f} x bound, {skipped} rows inside the margin")
    assert skipped <= 0.02 * N * A
    # exact given pred
    exp_correct = ((labels.long() >= 0) & (pred == labels.long())).to(torch.uint8)
    assert torch.equal(correct, exp_correct)
    assert torch.equal(n_correct.long(), exp_correct.long().sum(0))
    assert int(correct[0, 0]) == 0
    # without labels / logits: the same predictions, nothing else
    out2 = ops.cls_head(feats.cuda(), W1.cuda(), b1.cuda(), W2.cuda(), b2.cuda(), C)
    assert torch.equal(out2["pred"].cpu().long(), pred) and out2["logits"] is None and out2["correct"] is None


# ---- fixture classifiers ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fixture_classifiers_give_the_reference_names_and_logits(hip_lib):
    from multimodal_vae_comparison_amd import coherence as coh
    z = np.load(f"{COH_DIR}/classifier_cases.npz")
    nets = {}
    for att, C in (("shape", 3), ("color", 5)):
        nets[att] = coh.AttributeClassifier(C)
        nets[att].load_state_dict(load_fixture_classifier(att), strict=True)
    cls = coh.AttributeClassifiers(nets).cuda()
    images = torch.from_numpy(z["images"])
    x_hat = (images.float() / 255).cuda()      # what a decoder would hand over; predict() quantises it back to 8 bits
    out = cls.predict(x_hat, want_logits=True)
    names = cls.names(out["pred"])
    for i, att in enumerate(("shape", "color")):
        assert [n[i] for n in names] == [str(s) for s in z[f"names_{att}"]]
        ref = torch.from_numpy(z[f"logits_{att}"])
        got = out["logits"][i, :, :ref.shape[1]].cpu().double()
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"fixture classifier {att}: max logit error {err:.3e} of max |logit|")
        assert err <= 1e-5
        # one classifier alone, through its forward(): the same logits bit for bit
        assert torch.equal(nets[att](coh.quantise_images(x_hat)), out["logits"][i, :, :ref.shape[1]])


# ---- end to end -------------------------------------------------------------------------------------------------------
E2E_B, E2E_T, E2E_D, E2E_LEVEL = 6, 9, 8, 2
E2E_CAPTIONS = ["big heart", "heart", "square", "big", "small", "ellipse"]
E2E_MODS = [{"enc": "CNN2", "dec": "CNN", "data_dim": [64, 64, 3], "ltype": "bce"},
            {"enc": "TxtTransformer", "dec": "TxtTransformer", "data_dim": [E2E_T, 27, 1], "ltype": "category_ce"}]
DRAWS_PER_FORWARD = {"mopoe": 2, "poe": 1}


def _e2e_model(mixing):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import config_from_mods
    torch.manual_seed(11)
    cfg, dims = config_from_mods(mixing, E2E_MODS, E2E_D, batch_size=E2E_B)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0")
    tr.model.eval()
    return tr


def _e2e_batch():
    from multimodal_vae_comparison_amd import coherence as coh
    g = torch.Generator().manual_seed(21)
    ids = torch.tensor([coh.text_to_ids(c, E2E_T) for c in E2E_CAPTIONS])
    lens = torch.tensor([len(c) for c in E2E_CAPTIONS])
    mask = torch.arange(E2E_T)[None, :] < lens[:, None]
    onehot = F.one_hot(ids, 27).float() * mask[..., None]
    return {"mod_1": {"data": torch.rand(E2E_B, 3, 64, 64, generator=g).cuda(), "masks": None, "categorical": False},
            "mod_2": {"data": onehot.cuda(), "masks": mask.cuda(), "categorical": True}}


def _classifier_fp64(net, x):
    """the classifier in torch fp64 on the host -> logits (N,C)"""
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    h = x.double().cpu()
    for layer in ("conv1", "conv2", "conv3", "conv_64"):
        h = F.relu(F.conv2d(h, sd[f"{layer}.module.weight"], sd[f"{layer}.module.bias"], stride=2, padding=1))
    h = F.relu(F.linear(h.reshape(h.shape[0], -1), sd["lin1.module.weight"], sd["lin1.module.bias"]))
    return F.linear(h, sd["fc.module.weight"], sd["fc.module.bias"])


def _score_images_fp64(cls, level, x_hat, captions):
    """(strict, features) per sample from the fp64 classifiers; every argmax must be clear of the margin (with 6 rows
    the 2 % cap allows none inside it)"""
    from multimodal_vae_comparison_amd import coherence as coh
    x = torch.floor(x_hat.detach().float().cpu() * 255.0) / 255.0
    x = x.reshape(-1, 3, 64, 64)
    atts = coh.LEVEL_ATTRIBUTES[level]
    ok = torch.zeros(x.shape[0], dtype=torch.long)
    for i, a in enumerate(atts):
        logits = _classifier_fp64(cls.nets[a], x)
        top = logits.topk(2, dim=-1).values
        assert bool(((top[:, 0] - top[:, 1]) > 2.0 * 1e-5 * logits.abs().max()).all()), "an argmax inside the margin"
        pred = logits.argmax(-1)
        want = torch.tensor([coh.caption_labels(level, c)[i] for c in captions])
        ok += ((want >= 0) & (pred == want)).long()
    return [int(k == len(atts)) for k in ok.tolist()], [k / len(atts) for k in ok.tolist()]


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


@pytest.mark.gpu
@pytest.mark.parametrize("mixing", ["mopoe", "poe"])
def test_coherence_end_to_end(hip_lib, mixing):
    from multimodal_vae_comparison_amd import coherence as coh
    tr = _e2e_model(mixing)
    model = tr.model
    torch.manual_seed(5)
    cls = coh.AttributeClassifiers.for_level(E2E_LEVEL).cuda()
    batch = _e2e_batch()
    B, T, D, level = E2E_B, E2E_T, E2E_D, E2E_LEVEL
    g = torch.Generator().manual_seed(31)
    n_draws = 2 * DRAWS_PER_FORWARD[mixing]
    eps = [torch.randn(B, D, generator=g) for _ in range(n_draws)]
    eps_joint = torch.randn(16, D, generator=g)
    # a gradient to watch: one objective + backward before the evaluation
    model.objective(batch)["loss"].backward()
    torch.cuda.synchronize()
    before = _state(model)

    out = tr.cross_coherence([batch], cls, level, eps=[e.clone() for e in eps])
    joint = tr.joint_coherence(cls, level, n=16, eps=eps_joint.clone())
    torch.cuda.synchronize()
    _same_state(before, _state(model))
    assert model.eps_override is None and model._eval_draws is False
    assert out["captions"] == E2E_CAPTIONS

    # ---- the recomputation: forward()'s own decoder outputs, the fixture-checked text semantics, fp64 classifiers ----
    with torch.no_grad():
        model.eps_override = [e.clone() for e in eps]
        o1 = model.forward(model._given_only(batch, ["mod_2"]))
        x_hat = o1.mods["mod_1"].decoder_dist.loc
        x2 = model._given_only(batch, ["mod_1"])
        x2["mod_2"] = dict(x2["mod_2"], masks=None)
        logits = model.forward(x2).mods["mod_2"].decoder_dist.loc.reshape(B, T, 27)
        assert model.eps_override == []
        model.eps_override = None
    strict, feats = _score_images_fp64(cls, level, x_hat, E2E_CAPTIONS)
    assert out["per_sample"]["text_image_strict"] == strict
    assert out["per_sample"]["text_image_features"] == feats
    assert out["text_image"] == [100.0 * sum(strict) / B, 100.0 * sum(feats) / B]
    decoded = [coh.ids_to_text(r) for r in torch.argmax(logits, -1).cpu().tolist()]
    assert out["decoded"] == decoded
    triples = [coh.score_decoded_text(level, c, d) for c, d in zip(E2E_CAPTIONS, decoded)]
    assert out["per_sample"]["image_text_strict"] == [t[0] for t in triples]
    assert out["per_sample"]["image_text_features"] == [t[1] for t in triples]
    assert out["per_sample"]["image_text_letters"] == [t[2] for t in triples]
    assert out["image_text"] == [100.0 * sum(t[i] for t in triples) / B for i in range(3)]
    for name, v in (("text_image_strict", out["text_image"][0]), ("image_text_letters", out["image_text"][2])):
        assert float(tr.logged[f"test_coherence_{name}"]) == v

    with torch.no_grad():
        loc, scale = model.pz_params
        zj = (loc + scale * eps_joint.cuda()).unsqueeze(0)
        xj = model.vaes["mod_1"].dec({"latents": zj, "masks": None})[0]
        lj = model.vaes["mod_2"].dec({"latents": zj, "masks": None})[0].reshape(16, T, 27)
    dj = [coh.ids_to_text(r) for r in torch.argmax(lj, -1).cpu().tolist()]
    assert joint["decoded"] == dj
    atts = [coh.retrieve_attributes(t, level) for t in dj]
    assert joint["attributes"] == atts
    js, jf = _score_images_fp64(cls, level, xj, atts)
    assert joint["per_sample"] == {"joint_strict": js, "joint_features": jf}
    assert joint["joint"] == [100.0 * sum(js) / 16, 100.0 * sum(jf) / 16]
    assert float(tr.logged["test_coherence_joint_features"]) == joint["joint"][1]

    # a second call with the same noise: bit-identical
    out2 = model.cross_coherence([batch], cls, level, eps=[e.clone() for e in eps])
    joint2 = model.joint_coherence(cls, level, n=16, eps=eps_joint.clone())
    assert out2 == out and joint2 == joint

    # the generator path: the evaluation generator moves, the training one does not
    ev = model._eval_rng_state.clone()
    model.cross_coherence([batch], cls, level)
    model.joint_coherence(cls, level, n=5)
    torch.cuda.synchronize()
    assert not torch.equal(model._eval_rng_state, ev)
    _same_state(before, _state(model))
