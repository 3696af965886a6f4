"""csrc/text_quality.hip and TorchMMVAE.text_quality on the MI355X, held to the plain Python / numpy
restatement of tests/text_quality_reference.py (checked on the host against a memoised recursion, worked examples and torch's
float64 cross_entropy): every integer output equal, the negative log-likelihood within the bar that module derives.  Every call
runs twice and must give the same bits.  Nothing is held to the code under test."""
import numpy as np
import pytest
import torch

import text_quality_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def same_bits(a, b):
    """two ops.text_quality results, bit for bit"""
    for name in ("token", "word"):
        if (a[name] is None) != (b[name] is None):
            return False
        if a[name] is not None and (set(a[name]) != set(b[name]) or not all(torch.equal(a[name][k], b[name][k]) for k in a[name])):
            return False
    for name in ("pred", "nll", "nll_steps"):
        if (a[name] is None) != (b[name] is None) or (a[name] is not None and not torch.equal(a[name], b[name])):
            return False
    return a["max_order"] == b["max_order"]


def held(got, ref, what):
    """the integer outputs equal the restatement's, nll within its bar (printed first)"""
    N = len(ref["token"]["edit"])
    K = ref["max_order"]
    assert set(got) == {"token", "word", "pred", "nll", "nll_steps", "max_order"} and got["max_order"] == K
    for lvl, keys in (("token", R.TOKEN_KEYS), ("word", R.WORD_KEYS)):
        if ref[lvl] is None:
            assert got[lvl] is None, (what, lvl)
            continue
        assert set(got[lvl]) == set(keys), (what, lvl)
        for k in keys:
            g = got[lvl][k]
            assert g.dtype == torch.int32 and g.device.type == "cuda" and tuple(g.shape) == ((N, 4) if k in ("match", "total") else (N,))
            assert np.array_equal(g.cpu().numpy(), ref[lvl][k]), (what, lvl, k, g.cpu().numpy(), ref[lvl][k])
        assert not got[lvl]["match"][:, K:].any() and not got[lvl]["total"][:, K:].any(), (what, "columns >= max_order")
    if ref["pred"] is None:
        assert got["pred"] is None and got["nll"] is None and got["nll_steps"] is None
        return
    assert got["pred"].dtype == torch.int32 and np.array_equal(got["pred"].cpu().numpy(), ref["pred"]), what
    assert got["nll_steps"].dtype == torch.int32 and np.array_equal(got["nll_steps"].cpu().numpy(), ref["nll_steps"]), what
    assert got["nll"].dtype == torch.float64
    nll = got["nll"].cpu().numpy()
    zero = ref["nll_steps"] == 0
    assert np.all(nll[zero] == 0.0), (what, "no scored step must give exactly 0")
    if (~zero).any():
        e = np.abs(nll[~zero] - ref["nll"][~zero]) / ref["bar"][~zero]
        print(f"{what}: nll off by {e.max():.3g} bars (largest bar {ref['bar'].max():.3g})")
        assert e.max() <= 1.0, (what, e)


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_against_the_restatement(ops, i):
    c, ref = R.case(i)
    args = (dev(c["hyp"]), dev(c["ref"]), dev(c["ref_len"]), dev(c["hyp_len"]))
    got = ops.text_quality(*args, **c["kw"])
    held(got, ref, R.IDS[i])
    assert same_bits(got, ops.text_quality(*args, **c["kw"])), "two calls differ"
    if got["pred"] is not None:      # the ids form of the same hypothesis
        ids = ops.text_quality(got["pred"], *args[1:], **c["kw"])
        assert ids["pred"] is None and ids["nll"] is None and ids["nll_steps"] is None
        assert same_bits(dict(got, pred=None, nll=None, nll_steps=None), ids), "the ids form and the logits form differ"


def test_input_forms(ops):
    """any integer dtype, logits of any float dtype read as fp32, views that are not contiguous"""
    c, ref = R.case(R.IDS.index("logits_45_vs_32"))
    x, r, rl = dev(c["hyp"]), dev(c["ref"]), dev(c["ref_len"])
    want = ops.text_quality(x, r, rl, **c["kw"])
    held(want, ref, "logits_45_vs_32")
    assert same_bits(want, ops.text_quality(x.double(), r.int(), rl.short(), **c["kw"]))
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)
    rt = r.t().contiguous().t()
    assert not xt.is_contiguous() and not rt.is_contiguous() and same_bits(want, ops.text_quality(xt, rt, rl, **c["kw"]))
    full = torch.full_like(rl, x.shape[1])
    assert same_bits(want, ops.text_quality(x, r, rl, full, **c["kw"])), "hyp_lengths = Th is the default"
    for match, args, kw in (("ref_ids holds ids from", (x, r + 27, rl), {}), ("one device", (x, r.cpu(), rl), {})):
        with pytest.raises(ValueError, match="text_quality: .*" + match):
            ops.text_quality(*args, **kw)


# ---- 2. against the existing kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", "vocab_256", "vocab_2", "hyp_lengths"])
def test_against_text_decode_score(ops, name):
    c, _ = R.case(R.IDS.index(name))
    x, r, rl = dev(c["hyp"]), dev(c["ref"]), dev(c["ref_len"])
    T = min(x.shape[1], r.shape[1])
    x, r = x[:, :T].contiguous(), r[:, :T].int().contiguous()      # equal step counts
    pred, letters = ops.text_decode_score(x, r, rl.int())
    got = ops.text_quality(x, r, rl)                                # eos and trim off
    assert torch.equal(got["pred"], pred) and torch.equal(got["token"]["same"], letters)
    assert torch.equal(got["token"]["ref_len"], rl.clamp(0, T).int()) and bool((got["token"]["hyp_len"] == T).all())


# ---- 3. a pair does not depend on its neighbours ------------------------------------------------------------------------------------
def test_a_pair_is_scored_alone(ops):
    rng = np.random.default_rng(21)
    N, Th, Tr, V = 301, 45, 40, 27
    hyp, ref, rl, _ = R._pairs(N, Th, Tr, V, rng)
    x = dev(R.as_logits(hyp, V, rng))
    r, rl = dev(ref), dev(rl)
    kw = dict(trim=0, sep=0)
    full = ops.text_quality(x, r, rl, **kw)
    assert same_bits(full, ops.text_quality(x, r, rl, **kw))
    rows = lambda d, s: None if d is None else {k: v[s] for k, v in d.items()}
    cut = lambda s: dict(full, token=rows(full["token"], s), word=rows(full["word"], s), pred=full["pred"][s], nll=full["nll"][s],
                         nll_steps=full["nll_steps"][s])
    for s in (slice(0, 5), slice(299, None), slice(150, 151)):      # (the last: N = 1)
        alone = ops.text_quality(x[s].contiguous(), r[s].contiguous(), rl[s].contiguous(), **kw)
        assert same_bits(alone, cut(s)), s
    some = [0, 1, 2, 150, 299, 300]
    ref5 = R.text_quality(x[some].cpu().numpy(), ref[some], rl[some].cpu().numpy(), **kw)
    held(ops.text_quality(x[some].contiguous(), r[some].contiguous(), rl[some].contiguous(), **kw), ref5, "rows of 301")
    ids = ops.text_quality(full["pred"][:1], r[:1], rl[:1], **kw)      # N = 1, ids form
    assert torch.equal(ids["token"]["edit"], full["token"]["edit"][:1]) and torch.equal(ids["word"]["lcs"], full["word"]["lcs"][:1])


# ---- 4. the metric end to end -------------------------------------------------------------------------------------------------------
T_E2E, V_E2E, B_E2E, D_E2E = 12, 27, 8, 8
MODS = [{"enc": "CNN2", "dec": "CNN", "data_dim": [64, 64, 3], "ltype": "bce"},
        {"enc": "TxtTransformer", "dec": "TxtTransformer", "data_dim": [T_E2E, V_E2E, 1], "ltype": "category_ce"}]


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


def _batch(seed):
    """an image and a caption of words over a small alphabet (id 0 the space), one-hot, with its mask"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 5, (B_E2E, T_E2E), generator=g)
    lens = torch.randint(3, T_E2E + 1, (B_E2E,), generator=g)
    lens[0] = T_E2E
    mask = torch.arange(T_E2E)[None, :] < lens[:, None]
    onehot = torch.nn.functional.one_hot(ids, V_E2E).float() * mask[..., None]
    return {"mod_1": {"data": torch.rand(B_E2E, 3, 64, 64, generator=g).to(DEV), "masks": None, "categorical": False},
            "mod_2": {"data": onehot.to(DEV), "masks": mask.to(DEV), "categorical": True}}, ids * mask, lens


@pytest.mark.parametrize("mixing", ["poe", "moe"])
def test_text_quality_end_to_end(ops, mixing):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import config_from_mods
    B, T, V = B_E2E, T_E2E, V_E2E
    torch.manual_seed(41)
    cfg, dims = config_from_mods(mixing, MODS, D_E2E, batch_size=B)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    made = [_batch(s) for s in (43, 44)]
    batches = [b for b, _, _ in made]
    g = torch.Generator().manual_seed(45)
    eps = [torch.randn(B, D_E2E, generator=g) for _ in range(32)]
    model.objective(batches[0])["loss"].backward()      # a gradient to watch
    torch.cuda.synchronize()
    before = _state(model)

    out = model.text_quality(batches, eps=[e.clone() for e in eps])
    torch.cuda.synchronize()
    _same_state(before, _state(model))
    assert model.eps_override is None and model._eval_draws is False and torch.is_grad_enabled()
    assert set(out) == {"mod_2"}
    r = out["mod_2"]
    assert set(r) == {"recon", "cross", "n", "per_sample"} and r["n"] == 2 * B
    assert set(r["cross"]) == {"mod_1"} and set(r["per_sample"]) == {"recon", "cross"} and set(r["per_sample"]["cross"]) == {"mod_1"}

    # ---- the same forward() calls by hand: the full batch, then only the image given with the text masks None -----------
    recon, cross = [], []
    with torch.no_grad():
        model.eps_override = [e.clone() for e in eps]
        for b in batches:
            recon.append(model.forward(b).mods["mod_2"].decoder_dist.loc.reshape(-1, T, V)[:B].float().contiguous())
            x = model._given_only(b, ["mod_1"])
            x["mod_2"] = dict(x["mod_2"], masks=None)
            cross.append(model.forward(x).mods["mod_2"].decoder_dist.loc.reshape(-1, T, V)[:B].float().contiguous())
        model.eps_override = None
    ids = torch.cat([i for _, i, _ in made])
    lens = torch.cat([l for _, _, l in made])
    kw = dict(trim=0, sep=0)
    refs = {}
    for what, logits, S, P in (("recon", torch.cat(recon), r["recon"], r["per_sample"]["recon"]),
                               ("cross", torch.cat(cross), r["cross"]["mod_1"], r["per_sample"]["cross"]["mod_1"])):
        by_hand = ops.text_quality(logits, ids.to(DEV), lens.to(DEV), **kw)
        assert same_bits(P, by_hand), (mixing, what)
        refs[what] = ref = R.text_quality(logits.cpu().numpy(), ids.numpy(), lens.numpy(), **kw)
        held(P, ref, f"{mixing} {what}")
        R.assert_same_summary(S, R.summary([ref | {"nll": P["nll"].cpu().numpy()}]))
        assert S["token"]["n"] == S["word"]["n"] == 2 * B and S["token"]["perplexity"] > 1.0
    # the reconstruction keeps its masks: nothing is decoded past a caption's end, so no hypothesis is longer than it
    assert bool((r["per_sample"]["recon"]["token"]["hyp_len"] <= lens.to(DEV)).all())
    assert not np.array_equal(refs["recon"]["pred"], refs["cross"]["pred"]), "the two sets decode alike: choose another seed"

    with pytest.raises(ValueError, match="text_quality: `batches` is empty"):
        model.text_quality([])
    model.train()
    with pytest.raises(RuntimeError, match="text_quality needs eval mode"):
        model.text_quality(batches)
    model.eval()


def test_a_model_without_a_text_tower_refuses(ops):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import MS_MODS, config_from_mods, mnist_svhn_batch
    cfg, dims = config_from_mods("moe", MS_MODS, 8, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    with pytest.raises(ValueError, match=r"text_quality: no modality of this model is a text tower .*\(28, 28, 1\), \(32, 32, 3\)"):
        model.text_quality([mnist_svhn_batch(4, seed=5, device=DEV)])
