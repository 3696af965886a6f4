"""Host checks of the text generation quality.  The restatement the GPU tests of csrc/text_quality.hip are
held to (tests/text_quality_reference.py) against independent routes -- a memoised recursion for the two alignments, worked
examples counted by hand, torch's float64 cross_entropy for the negative log-likelihood --, the summary arithmetic of
ops.text_quality_summary on counts computed by hand, the ABI of the new entry points, and what ops.text_quality and
TorchMMVAE.text_quality refuse before anything reaches a kernel."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import text_quality_reference as R
from conftest import ROOT

SYMBOLS = ("mmvae_text_quality", "mmvae_text_quality_lds_bytes")


def chars(s):
    """' ' -> 0, a .. z -> 1 .. 26"""
    return [0 if c == " " else ord(c) - 96 for c in s]


# ---- 1. the restatement against independent routes ----------------------------------------------------------------------------------
def _recursive(a, b):
    """(edit distance, LCS length) by the textbook recursions on prefixes, memoised"""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return max(i, j)
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))

    @functools.lru_cache(maxsize=None)
    def c(i, j):
        if i == 0 or j == 0:
            return 0
        return c(i - 1, j - 1) + 1 if a[i - 1] == b[j - 1] else max(c(i - 1, j), c(i, j - 1))

    return d(len(a), len(b)), c(len(a), len(b))


def test_alignments_against_the_memoised_recursion():
    rng = np.random.default_rng(0)
    for _ in range(300):
        a = [int(v) for v in rng.integers(0, 4, int(rng.integers(0, 13)))]
        b = [int(v) for v in rng.integers(0, 4, int(rng.integers(0, 13)))] if rng.random() < 0.7 else R.noisy(a, rng, 4)
        assert (R.levenshtein(a, b), R.lcs(a, b)) == _recursive(a, b), (a, b)
    words = [(1, 2), (3,), (1, 2), (4, 4, 4)]
    assert (R.levenshtein(words, words[1:]), R.lcs(words, words[1:])) == (1, 3)


def test_papineni_example():
    """the the the the the the the / the cat is on the mat: the unigram is clipped at the reference's two"""
    the, cat, is_, on, mat = 1, 2, 3, 4, 5
    r = R.text_quality(np.array([[the] * 7]), np.array([[the, cat, is_, on, the, mat, 0]]), [6])["token"]
    assert r["match"].tolist() == [[2, 0, 0, 0]] and r["total"].tolist() == [[7, 6, 5, 4]]
    assert (int(r["edit"][0]), int(r["lcs"][0]), int(r["hyp_len"][0]), int(r["ref_len"][0])) == (5, 2, 7, 6)
    assert int(r["same"][0]) == 2      # positions 0 and 4


def test_caption_example():
    ref, hyp = "small red heart at top left", "small red hart at top  left   "
    r = R.text_quality(np.array([chars(hyp)]), np.array([chars(ref) + [0] * 3]), [len(ref)], trim=0, sep=0)
    t, w = r["token"], r["word"]
    assert (int(t["hyp_len"][0]), int(t["ref_len"][0]), int(t["edit"][0]), int(t["lcs"][0])) == (27, 27, 2, 26)
    assert t["match"].tolist() == [[26, 24, 21, 18]] and t["total"].tolist() == [[27, 26, 25, 24]]
    assert int(t["same"][0]) == len("small red h") + len(" left")      # (the two shifts cancel at the last word)
    assert (int(w["hyp_len"][0]), int(w["ref_len"][0]), int(w["edit"][0]), int(w["lcs"][0])) == (6, 6, 1, 5)
    assert w["match"].tolist() == [[5, 3, 1, 0]] and w["total"].tolist() == [[6, 5, 4, 3]] and "same" not in w


def test_cut_and_words():
    assert R.cut([1, 2, 3, 4], 9) == [1, 2, 3, 4] and R.cut([1, 2, 3, 4], -1) == [] and R.cut([1, 2, 3, 4], 2) == [1, 2]
    assert R.cut([1, 0, 3, 0, 0], 5, eos=3, trim=0) == [1] and R.cut([3, 1], 2, eos=3) == [] and R.cut([0, 0], 2, trim=0) == []
    assert R.cut([1, 3, 0, 0], 4, eos=None, trim=0) == [1, 3]
    assert R.words([0, 0, 1, 2, 0, 0, 3, 0], 0) == [(1, 2), (3,)] and R.words([0, 0], 0) == [] and R.words([5], 0) == [(5,)]
    k = R.text_quality(np.array([[1, 2, 1, 2, 1]]), np.array([[1, 2, 1, 9, 9]]), [3], max_order=2)["token"]
    assert k["match"].tolist() == [[3, 2, 0, 0]] and k["total"].tolist() == [[5, 4, 0, 0]]


LOGIT_CASES = [i for i, name in enumerate(R.IDS) if R.case(i)[0]["hyp"].ndim == 3]


@pytest.mark.parametrize("i", LOGIT_CASES, ids=[R.IDS[i] for i in LOGIT_CASES])
def test_nll_against_torch_cross_entropy(i):
    c, ref = R.case(i)
    x = torch.from_numpy(np.array(c["hyp"])).double()
    N, Th, V = x.shape
    worst = 0.0
    for n in range(N):
        S = int(ref["nll_steps"][n])
        assert S == min(min(max(int(c["ref_len"][n]), 0), c["ref"].shape[1]), Th)
        if S == 0:
            assert ref["nll"][n] == 0.0 and ref["bar"][n] == 0.0
            continue
        target = torch.from_numpy(np.array(c["ref"][n, :S])).long()
        other = float(torch.nn.functional.cross_entropy(x[n, :S], target, reduction="sum"))
        worst = max(worst, abs(other - ref["nll"][n]) / ref["bar"][n])
    print(f"{R.IDS[i]}: nll of the two routes {worst:.3g} bars (largest bar {ref['bar'].max():.3g})")
    assert worst <= 1.0
    assert np.array_equal(ref["pred"], torch.argmax(x, -1).numpy())


# ---- 2. the summary ------------------------------------------------------------------------------------------------------------------
def _part(token, word=None, nll=None, steps=None, K=4):
    t = lambda d: None if d is None else {k: torch.tensor(v, dtype=torch.int32) for k, v in d.items()}
    return {"token": t(token), "word": t(word), "pred": None, "nll": None if nll is None else torch.tensor(nll, dtype=torch.float64),
            "nll_steps": None if steps is None else torch.tensor(steps, dtype=torch.int32), "max_order": K}


def test_summary_on_counts_computed_by_hand():
    from multimodal_vae_comparison_amd import ops
    a = _part({"hyp_len": [4], "ref_len": [5], "same": [3], "edit": [2], "lcs": [3], "match": [[3, 1, 0, 0]],
               "total": [[4, 3, 0, 0]]}, nll=[2.0], steps=[4], K=2)
    b = _part({"hyp_len": [0], "ref_len": [2], "same": [0], "edit": [2], "lcs": [0], "match": [[0, 0, 0, 0]],
               "total": [[0, 0, 0, 0]]}, nll=[1.0], steps=[2], K=2)
    s = ops.text_quality_summary([a, b])
    assert s["word"] is None
    t = s["token"]
    close = lambda x, y: abs(x - y) <= 8 * 2.0 ** -53 * max(abs(y), 1.0)      # a handful of roundings each
    assert t["n"] == 2 and t["error_rate"] == 4 / 7 and t["exact"] == 0.0 and t["accuracy"] == 3 / 7
    assert t["precisions"] == [3 / 4, 1 / 3]
    assert close(t["bleu"], math.exp(1 - 7 / 4) * math.sqrt(3 / 4 * 1 / 3))
    assert close(t["sentence_bleu"], 0.5 * math.exp(1 - 5 / 4) * math.sqrt(3 / 4 * 2 / 4))      # the empty hypothesis scores 0
    assert close(t["rouge_l"], 0.5 * (2 * 0.75 * 0.6 / 1.35))
    assert t["nll"] == 0.5 and close(t["perplexity"], math.exp(0.5)) and close(t["bits_per_token"], 0.5 / math.log(2))
    # one part alone: no brevity penalty when the hypothesis is the longer one
    long = _part({"hyp_len": [6], "ref_len": [5], "same": [5], "edit": [1], "lcs": [5], "match": [[5, 4, 3, 2]],
                  "total": [[6, 5, 4, 3]]}, word={"hyp_len": [2], "ref_len": [2], "edit": [0], "lcs": [2], "match": [[2, 1, 0, 0]],
                                                  "total": [[2, 1, 0, 0]]})
    s = ops.text_quality_summary(long)
    assert close(s["token"]["bleu"], (5 / 6 * 4 / 5 * 3 / 4 * 2 / 3) ** 0.25) and s["token"]["perplexity"] is None
    assert close(s["token"]["sentence_bleu"], (5 / 6 * 5 / 6 * 4 / 5 * 3 / 4) ** 0.25)
    # a word level whose 3-gram sum is 0: corpus BLEU is 0, the smoothed sentence BLEU is not
    w = s["word"]
    assert w["bleu"] == 0.0 and w["exact"] == 1.0 and w["error_rate"] == 0.0 and w["rouge_l"] == 1.0 and "accuracy" not in w
    assert close(w["sentence_bleu"], (1.0 * 1.0 * 1.0 * 1.0) ** 0.25) and w["precisions"] == [1.0, 1.0, 0.0, 0.0]
    # no unigram match: the pair's sentence BLEU is 0; nothing to divide by: 0, or inf for errors against empty references
    none = _part({"hyp_len": [3], "ref_len": [0], "same": [0], "edit": [3], "lcs": [0], "match": [[0, 0, 0, 0]],
                  "total": [[3, 2, 1, 0]]})
    t = ops.text_quality_summary([none])["token"]
    assert (t["bleu"], t["sentence_bleu"], t["rouge_l"], t["accuracy"]) == (0.0, 0.0, 0.0, 0.0) and t["error_rate"] == math.inf
    with pytest.raises(ValueError, match="text_quality_summary: the parts were scored with different"):
        ops.text_quality_summary([a, long])
    with pytest.raises(ValueError, match="text_quality_summary: no parts"):
        ops.text_quality_summary([])


@pytest.mark.parametrize("name", ["logits_45_vs_32", "eos_trim", "words", "order_1"])
def test_summary_against_the_restatement(name):
    from multimodal_vae_comparison_amd import ops
    _, ref = R.case(R.IDS.index(name))
    t = lambda d: None if d is None else {k: torch.from_numpy(np.array(v)) for k, v in d.items()}
    part = {"token": t(ref["token"]), "word": t(ref["word"]), "pred": None,
            "nll": None if ref["nll"] is None else torch.from_numpy(ref["nll"]),
            "nll_steps": None if ref["nll"] is None else torch.from_numpy(ref["nll_steps"]), "max_order": ref["max_order"]}
    R.assert_same_summary(ops.text_quality_summary([part]), R.summary([ref]))
    half = lambda d, s: None if d is None else {k: v[s] for k, v in d.items()}
    n = len(ref["token"]["edit"]) // 2
    halves = [dict(part, token=half(part["token"], s), word=half(part["word"], s),
                   nll=None if part["nll"] is None else part["nll"][s],
                   nll_steps=None if part["nll"] is None else part["nll_steps"][s]) for s in (slice(0, n), slice(n, None))]
    R.assert_same_summary(ops.text_quality_summary(halves), R.summary([ref]))


# ---- 3. the ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from multimodal_vae_comparison_amd import hipops
    from multimodal_vae_comparison_amd.models.vae import MIXER_METRICS
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES, f"{name} is not in the ctypes table"
        assert hasattr(hipops.lib(), name)
    for macro, value in (("MMVAE_TQ_MAX_STEPS", hipops.TQ_MAX_STEPS), ("MMVAE_TQ_MAX_VOCAB", hipops.TQ_MAX_VOCAB),
                         ("MMVAE_TQ_MAX_ORDER", hipops.TQ_MAX_ORDER), ("MMVAE_TQ_MAX_ROWS", hipops.TQ_MAX_ROWS)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value, macro
    assert (hipops.TQ_MAX_STEPS, hipops.TQ_MAX_VOCAB) == (256, 256)
    assert "text_quality" in MIXER_METRICS
    assert "text_quality.hip" in open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "Makefile")).read()


def test_pure_query_and_refusals_of_the_entry_point_run_without_gpu():
    from multimodal_vae_comparison_amd import hipops
    L = hipops.lib()
    b = L.mmvae_text_quality_lds_bytes
    assert b(45, 45) == b(256, 256) == b(1, 256) > 0 and 32 * b(256, 256) <= 160 * 1024      # 32 single-wave workgroups a CU
    assert (b(0, 45), b(45, 0), b(257, 45), b(45, 257)) == (0, 0, 0, 0)
    one = (hipops.c_i * 16)()
    dbl = (hipops.ctypes.c_double * 1)()
    p = lambda a: hipops.ctypes.cast(a, hipops.c_p)
    call = lambda logits, hyp, word, Th, Tr, V, sep, K, N=1: L.mmvae_text_quality(
        logits, hyp, p(one), p(one), None, p(one), p(one), word, p(dbl), p(one), N, Th, Tr, V, -1, -1, sep, K, None)
    # MMVAE_ERR_ARG (1): no hypothesis; a separator without the word output and the reverse.  Nothing is launched.
    assert call(None, None, None, 4, 4, 4, -1, 4) == 1
    assert call(None, p(one), None, 4, 4, 4, 0, 4) == 1 and call(None, p(one), p(one), 4, 4, 4, -1, 4) == 1
    # MMVAE_ERR_UNSUPPORTED (2): outside the limits
    for Th, Tr, V, K, N in ((0, 4, 4, 4, 1), (257, 4, 4, 4, 1), (4, 0, 4, 4, 1), (4, 257, 4, 4, 1), (4, 4, 1, 4, 1),
                            (4, 4, 257, 4, 1), (4, 4, 4, 0, 1), (4, 4, 4, 5, 1), (4, 4, 4, 4, 0), (4, 4, 4, 4, 2 ** 26), (4, 4, 4, 4, 2 ** 31)):
        assert call(None, p(one), None, Th, Tr, V, -1, K, N) == 2, (Th, Tr, V, K, N)


# ---- 4. the op's refusals, before any device call ---------------------------------------------------------------------------------
def test_ops_refuse_before_a_device_call():
    from multimodal_vae_comparison_amd import ops
    x = torch.randn(2, 5, 7)
    ids = torch.randint(0, 7, (2, 5))
    lens = torch.tensor([5, 3])
    cases = [
        ("hyp is list", ([1], ids, lens), {}),
        (r"hyp is \(2, 5\), torch.float32", (x[:, :, 0], ids, lens), {}),
        (r"hyp is \(2, 5, 7\), torch.int64", (x.long(), ids, lens), {}),
        (r"ref_ids is \(2,\)", (x, lens, lens), {}),
        ("ref_ids is .*torch.float32; integers", (x, ids.float(), lens), {}),
        (r"ref_ids is \(3, 5\), not \(2, T\)", (x, torch.zeros(3, 5, dtype=torch.long), lens), {}),
        (r"ref_lengths is \(3,\), not \(2,\)", (x, ids, torch.tensor([1, 2, 3])), {}),
        ("ref_lengths is .*torch.bool", (x, ids, torch.tensor([True, False])), {}),
        (r"hyp_lengths is \(2, 1\)", (x, ids, lens, lens[:, None]), {}),
        ("0 pairs", (x[:0], ids[:0], lens[:0]), {}),
        ("hypotheses of 257 steps", (torch.zeros(1, 257, 4), ids[:1], lens[:1]), {}),
        ("references of 300", (x, torch.zeros(2, 300, dtype=torch.long), lens), {}),
        ("V = 1 ", (x[:, :, :1], torch.zeros(2, 5, dtype=torch.long), lens), {}),
        ("V = 257", (torch.zeros(1, 3, 257), ids[:1], lens[:1]), {}),
        ("max_order = 5", (x, ids, lens), {"max_order": 5}),
        ("max_order = 0", (x, ids, lens), {"max_order": 0}),
        (r"eos = 7 \(a token id in \[0, 7\)", (x, ids, lens), {"eos": 7}),
        ("trim = -1", (x, ids, lens), {"trim": -1}),
        ("sep = 1.5", (x, ids, lens), {"sep": 1.5}),
        ("sep = eos = 2", (x, ids, lens), {"sep": 2, "eos": 2}),
        (r"ref_ids holds ids from 0 to 7 .*\[0, 7\)", (x, torch.tensor([[0, 7, 1, 1, 1], [1, 1, 1, 1, 1]]), lens), {}),
        (r"ref_ids holds ids from -1", (x, ids - 1 - ids, lens), {}),
        (r"hyp holds ids from 0 to 256 .*\[0, 256\)", (torch.tensor([[0, 256]]), torch.tensor([[1, 2]]), lens[:1]), {}),
        ("hyp is on cpu", (x, ids, lens), {}),
        ("hyp is on cpu", (ids, ids.int(), lens.short()), {"sep": 0, "trim": 0, "eos": 3}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="text_quality: .*" + match):
            ops.text_quality(*args, **kwargs)
    assert ops.text_quality_plan(45, 32, 27, None, 0, 0, 4) == {"eos": -1, "trim": 0, "sep": 0, "max_order": 4}


# ---- 5. the method's contract on CPU models -----------------------------------------------------------------------------------------
def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


def test_unimodal_vae_refuses_by_name():
    from multimodal_vae_comparison_amd.models.vae import VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE)
    with pytest.raises(NotImplementedError) as e:
        vae.text_quality()
    assert "unimodal" in str(e.value) and "TorchMMVAE.text_quality" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="text_quality needs eval mode"):
        model.text_quality([cdsprites_batch(4, 6, seed=3)])


def test_argument_errors_come_before_the_first_forward(monkeypatch):
    from multimodal_vae_comparison_amd import synthetic
    model = _model()
    batch = synthetic.cdsprites_batch(4, 6, seed=3)
    calls = []
    monkeypatch.setattr(model, "forward", lambda *a, **kw: calls.append(1))
    who = "text_quality: .*"
    for match, args, kwargs in [
            (who + "`batches` is empty", ([],), {}),
            (who + "without data", ([dict(batch, mod_1=dict(batch["mod_1"], data=None))],), {}),
            (who + "`texts` lists modalities", ([batch],), {"texts": []}),
            (who + "`texts` lists modalities", ([batch],), {"texts": ["mod_9"]}),
            (who + "`texts` lists modalities", ([batch],), {"texts": ["mod_2", "mod_2"]}),
            (who + r"'mod_1' must be one-hot \(B, T, V\)", ([batch],), {"texts": ["mod_1"]}),
            (who + "max_order = 7", ([batch],), {"max_order": 7}),
            (who + "sep = 27", ([batch],), {"sep": 27}),
            (who + "sep = eos = 0", ([batch],), {"eos": 0}),
            (who + "references of 300 ",([synthetic.cdsprites_batch(4, 300, seed=3)],), {})]:
        with pytest.raises(ValueError, match=match):
            model.text_quality(*args, **kwargs)
    images_only = _model(mods=[synthetic.CD_MODS[0], dict(synthetic.CD_MODS[0])])
    with pytest.raises(ValueError, match=who + r"no modality of this model is a text tower .*\(64, 64, 3\), \(64, 64, 3\)"):
        images_only.text_quality([batch])
    long_text = _model(mods=[synthetic.CD_MODS[0], dict(synthetic.CD_MODS[1], data_dim=[300, 27, 1])])
    with pytest.raises(ValueError, match=who + r"no modality of this model is a text tower .*\(300, 27, 1\)"):
        long_text.text_quality([batch])
    assert not calls and model._eval_draws is False and model.eps_override is None
