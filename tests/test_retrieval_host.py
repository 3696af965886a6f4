"""Host checks of the cross-modal retrieval of latents.  The float64 restatement the GPU tests of
csrc/retrieval.hip are held to (tests/retrieval_reference.py) against cases worked by hand and against
torch.distributions.kl_divergence; the host-side arithmetic of ops.retrieval_summary and ops.retrieval_label_precision on
crafted integer inputs; the drop-in boundary (header, ctypes table, exports, constants, Makefile); the metric keeps the
contract of its neighbours on CPU models; the ops refuse what is outside the limits before any launch."""
import os
import re

import numpy as np
import pytest
import torch

import retrieval_reference as R
from conftest import ROOT

SYMBOLS = ("mmvae_retrieval_chunks", "mmvae_retrieval_ws_bytes", "mmvae_retrieval_ranks")


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------------
# three rows, D = 2, worked by hand: q0 = (0, 0), q1 = (1, 2), q2 = (3, 4) against g0 = (0, 0), g1 = (1, 0), g2 = (3, 4)
QL = np.array([[0, 0], [1, 2], [3, 4]], np.float32)
GL = np.array([[0, 0], [1, 0], [3, 4]], np.float32)
QS = np.array([[1, 1], [1, 2], [0.5, 1]], np.float32)
GS = np.array([[1, 1], [2, 1], [0.5, 1]], np.float32)
HAND = {
    "l2": [[0, 1, 25], [5, 4, 8], [25, 20, 0]],
    # 1 - q . g / (|q| |g|); a zero row gives 1
    "cosine": [[1, 1, 1], [1, 1 - 1 / 5 ** 0.5, 1 - 11 / (5 ** 0.5 * 5)], [1, 1 - 3 / 5, 0]],
    # + (sq - sg)^2
    "w2": [[0, 1 + 1, 25 + 0.25], [5 + 1, 4 + 1 + 1, 8 + 0.25 + 1], [25 + 0.25, 20 + 2.25, 0]],
}


def hand_skl(i, j):
    """sum_d 1/2 [(sq^2 + D^2) / sg^2 + (sg^2 + D^2) / sq^2] - 1 with Python floats"""
    out = 0.0
    for d in range(2):
        vq, vg, dd = float(QS[i, d]) ** 2, float(GS[j, d]) ** 2, (float(QL[i, d]) - float(GL[j, d])) ** 2
        out += 0.5 * ((vq + dd) / vg + (vg + dd) / vq) - 1.0
    return out


@pytest.mark.parametrize("metric", R.METRICS)
def test_restatement_against_a_case_worked_by_hand(metric):
    d, bar = R.pair_distances(metric, QL, QS, GL, GS)
    want = np.array(HAND[metric] if metric in HAND else [[hand_skl(i, j) for j in range(3)] for i in range(3)], np.float64)
    assert d.shape == bar.shape == (3, 3) and d.dtype == np.float64
    assert np.abs(d - want).max() <= 1e-15 * max(1.0, np.abs(want).max()), (d, want)
    assert np.all(bar >= 0) and np.all(bar <= 1e-13 * (1.0 + np.abs(want)))
    if metric == "skl":      # (by hand: q0 g0 are equal unit Gaussians; q0 g1: 1/2 [(1 + 1) / 4 + (4 + 1) / 1] - 1 + 0 = 1.75)
        assert d[0, 0] == 0.0 and d[0, 1] == 1.75
    if metric == "l2":
        dm, less, equal = R.ranks(d)
        assert dm.tolist() == [0, 4, 0] and less.tolist() == [0, 0, 0] and equal.tolist() == [0, 0, 0]
        dm, less, equal = R.ranks(d, np.array([2, 0, -1]))      # partners 2, 0 and none
        assert dm[:2].tolist() == [25, 5] and np.isnan(dm[2])
        assert less.tolist() == [2, 1, -1] and equal.tolist() == [0, 0, -1]
        nn_d, nn_idx = R.neighbours(d, 4)
        assert nn_idx.tolist() == [[0, 1, 2, -1], [1, 0, 2, -1], [2, 1, 0, -1]]
        assert nn_d[:, :3].tolist() == [[0, 1, 25], [4, 5, 8], [0, 20, 25]] and np.all(np.isinf(nn_d[:, 3]))


def test_restated_skl_is_torchs_kl_both_ways():
    rs = np.random.RandomState(5)
    ql, gl = rs.standard_normal((7, 5)).astype(np.float32), rs.standard_normal((9, 5)).astype(np.float32)
    qs, gs = rs.uniform(0.1, 1, (7, 5)).astype(np.float32), rs.uniform(0.1, 1, (9, 5)).astype(np.float32)
    d, bar = R.pair_distances("skl", ql, qs, gl, gs)
    q = torch.distributions.Normal(torch.from_numpy(ql).double()[:, None], torch.from_numpy(qs).double()[:, None])
    g = torch.distributions.Normal(torch.from_numpy(gl).double()[None], torch.from_numpy(gs).double()[None])
    kl = torch.distributions.kl_divergence
    want = (kl(q, g) + kl(g, q)).sum(-1).numpy()
    # torch's closed form takes logarithms that cancel between the two directions: a few more roundings than the bar counts
    assert np.all(np.abs(d - want) <= 4 * bar), float((np.abs(d - want) / bar).max())
    w2, _ = R.pair_distances("w2", ql, qs, gl, gs)
    l2, _ = R.pair_distances("l2", ql, None, gl, None)
    assert np.all(w2 > l2)


def test_ties_and_order_of_the_restatement():
    d = np.array([[1.0, 1.0, 0.5, 1.0], [2.0, 2.0, 2.0, 2.0]])
    dm, less, equal = R.ranks(d, np.array([1, 3]))
    assert dm.tolist() == [1, 2] and less.tolist() == [1, 0] and equal.tolist() == [2, 3]
    nn_d, nn_idx = R.neighbours(d, 3)
    assert nn_idx.tolist() == [[2, 0, 1], [0, 1, 2]]      # (by index within a tie)


def test_shared_cases_are_fair():
    """every (shape, metric) the GPU tests compare exactly passes `fair` from the restatement alone; cosine at D = 1 is all
    ties and belongs to the tie tests"""
    for N, D in R.SHAPES:
        for metric in R.METRICS:
            if metric == "cosine" and D == 1:
                continue
            r, c = R.reference(N, D, metric), R.case(N, D)
            assert R.fair(r["d"], r["bar"], c["match"], 16, f"{N} x {D} {metric}") >= 1e5
    r, c = R.reference(63, 1, "cosine"), R.case(63, 1)
    with pytest.raises(AssertionError, match="bars apart"):
        R.fair(r["d"], r["bar"], c["match"], 16)
    # a case with small noise is refused as trivial
    c = R.case(64, 8)
    d, bar = R.pair_distances("l2", c["loc"][0][c["match"]] + np.float32(1e-3), None, c["loc"][0], None)
    with pytest.raises(AssertionError, match="tells nothing"):
        R.fair(d, bar, c["match"], 4)


# ---- 2. the host-side arithmetic of the ops -----------------------------------------------------------------------------------------
def test_summary_is_pessimistic_and_leaves_out_rows_without_a_partner():
    from multimodal_vae_comparison_amd import ops
    less = torch.tensor([0, 0, 3, -1, 9, 1], dtype=torch.int32)
    equal = torch.tensor([0, 2, 0, -1, 0, 3], dtype=torch.int32)
    s = ops.retrieval_summary(less, equal, ks=(1, 3, 5), n_gallery=10)
    # ranks 1, 3, 4, (none), 10, 5
    assert s["n"] == 5 and s["tied_rows"] == 2
    assert s["recall@1"] == 1 / 5 and s["recall@3"] == 2 / 5 and s["recall@5"] == 4 / 5
    assert s["chance@1"] == 0.1 and s["chance@3"] == 0.3 and s["chance@5"] == 0.5
    assert s["median_rank"] == 4.0 and s["mean_rank"] == 23 / 5
    assert abs(s["mrr"] - (1 + 1 / 3 + 1 / 4 + 1 / 10 + 1 / 5) / 5) <= 1e-15
    assert abs(s["normalised_rank"] - (0 + 2 + 3 + 9 + 4) / 9 / 5) <= 1e-15
    want = R.summary(less.numpy(), equal.numpy(), (1, 3, 5), 10)
    assert s.keys() == want.keys() and all(abs(s[k] - want[k]) <= 1e-15 for k in s)
    # N identical embeddings: every other row ties -> rank N, recall 0 below N, the far end of the normalised rank
    N = 6
    s = ops.retrieval_summary(np.zeros(N, np.int32), np.full(N, N - 1, np.int32), ks=(1, 5, 6))
    assert s["recall@1"] == 0.0 and s["recall@5"] == 0.0 and s["recall@6"] == 1.0 and s["median_rank"] == N
    assert s["normalised_rank"] == 1.0 and s["tied_rows"] == N and s["chance@6"] == 1.0 and s["chance@5"] == 5 / 6
    # (P, N) counts give a list; one gallery row; no partner at all
    two = ops.retrieval_summary(torch.stack([less, less]), torch.stack([equal, equal]), ks=(1,), n_gallery=10)
    assert isinstance(two, list) and len(two) == 2 and two[0] == two[1] and two[0]["mrr"] == ops.retrieval_summary(
        less, equal, ks=(1,), n_gallery=10)["mrr"]
    one = ops.retrieval_summary([0], [0], ks=(1, 2))
    assert one["recall@1"] == 1.0 and one["normalised_rank"] == 0.0 and one["chance@2"] == 1.0
    none = ops.retrieval_summary([-1, -1], [-1, -1], ks=(1,), n_gallery=2)
    assert none["n"] == 0 and np.isnan(none["recall@1"]) and np.isnan(none["mrr"]) and none["chance@1"] == 0.5
    assert "pessimistic" in ops.retrieval_summary.__doc__.lower()
    for bad, match in ((([0, 1], [0], (1,)), "less is"), (([0, -1], [0, 0], (1,)), "disagree"), (([0], [0], ()), "ks ="),
                       (([0], [0], (0,)), "ks ="), (([0.5], [0], (1,)), "less is"), (([3, 0], [0, 0], (1,)), "n_gallery = 2")):
        with pytest.raises(ValueError, match="retrieval_summary: .*" + match):
            ops.retrieval_summary(bad[0], bad[1], ks=bad[2])


def test_label_precision_on_crafted_lists():
    from multimodal_vae_comparison_amd import ops
    nn_idx = np.array([[0, 1, 2], [2, 0, 1], [1, 2, -1]], np.int32)
    lq, lg = np.array([0, 1, 1]), np.array([0, 0, 1])
    # neighbour labels: [0 0 1] for label 0; [1 0 0] for label 1; [0 1 -] for label 1
    got = ops.retrieval_label_precision(nn_idx, lq, lg, ks=(1, 2, 3))
    assert got[1] == {"precision": (1 + 1 + 0) / 3, "hit": 2 / 3}
    assert got[2] == {"precision": (1 + 0.5 + 0.5) / 3, "hit": 1.0}
    assert abs(got[3]["precision"] - (2 / 3 + 1 / 3 + 1 / 2) / 3) <= 1e-15 and got[3]["hit"] == 1.0
    want = R.label_precision(nn_idx, lq, lg, (1, 2, 3))
    assert all(abs(got[k][n] - want[k][n]) <= 1e-15 for k in got for n in got[k])
    for args, match in (((nn_idx, lq, lg, (4,)), "keep = 3"), ((nn_idx, lq[:2], lg, (1,)), "labels_q"),
                        ((nn_idx, lq, lg[:2], (1,)), "outside"), ((nn_idx.astype(np.float32), lq, lg, (1,)), "nn_idx is")):
        with pytest.raises(ValueError, match="retrieval_label_precision: .*" + match):
            ops.retrieval_label_precision(*args[:3], ks=args[3])


# ---- 3. the drop-in boundary --------------------------------------------------------------------------------------------------------
def test_symbols_constants_and_wiring():
    from multimodal_vae_comparison_amd import hipops
    from multimodal_vae_comparison_amd.models.vae import MIXER_METRICS
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES, f"{name} is not in the ctypes table"
        assert hasattr(hipops.lib(), name)
    for macro, value in (("MMVAE_RETRIEVAL_MAX_ROWS", hipops.RETRIEVAL_MAX_ROWS), ("MMVAE_RETRIEVAL_MAX_DIM", hipops.RETRIEVAL_MAX_DIM),
                         ("MMVAE_RETRIEVAL_MAX_SETS", hipops.RETRIEVAL_MAX_SETS),
                         ("MMVAE_RETRIEVAL_MAX_PAIRS", hipops.RETRIEVAL_MAX_PAIRS),
                         ("MMVAE_RETRIEVAL_MAX_KEEP", hipops.RETRIEVAL_MAX_KEEP), ("MMVAE_RETRIEVAL_L2", hipops.RETRIEVAL_METRICS["l2"]),
                         ("MMVAE_RETRIEVAL_COSINE", hipops.RETRIEVAL_METRICS["cosine"]),
                         ("MMVAE_RETRIEVAL_W2", hipops.RETRIEVAL_METRICS["w2"]), ("MMVAE_RETRIEVAL_SKL", hipops.RETRIEVAL_METRICS["skl"])):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value, macro
    assert (hipops.RETRIEVAL_MAX_ROWS, hipops.RETRIEVAL_MAX_DIM, hipops.RETRIEVAL_MAX_SETS, hipops.RETRIEVAL_MAX_PAIRS,
            hipops.RETRIEVAL_MAX_KEEP) == (16384, 256, 16, 240, 16)
    assert "cross_modal_retrieval" in MIXER_METRICS
    assert "retrieval.hip" in open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "Makefile")).read()


def test_pure_queries_and_refusals_of_the_entry_point_run_without_gpu():
    from multimodal_vae_comparison_amd import hipops
    L = hipops.lib()
    chunks, ws = L.mmvae_retrieval_chunks, L.mmvae_retrieval_ws_bytes
    # ceil(1024 / (row tiles x P)) chunks, of 8 staged tiles of 32 rows at least
    assert chunks(10000, 2) == 4 and chunks(10000, 1) == 7 and chunks(200, 2) == 1 and chunks(16384, 240) == 1
    assert chunks(512, 1) == 2 and chunks(1, 1) == 1
    assert chunks(0, 1) == chunks(16385, 1) == chunks(10, 0) == chunks(10, 241) == 0
    assert ws(200, 2, 10, 0) == ws(200, 2, 10, 1) == 0      # (one chunk writes the outputs itself)
    assert ws(200, 2, 10, 3) == 3 * 2 * 200 * (10 * 12 + 8) and ws(200, 2, 0, 3) == 3 * 2 * 200 * 8
    assert ws(200, 2, 10, 1000) == ws(200, 2, 10, 7)        # (at most one chunk per staged tile)
    assert ws(200, 2, 17, 3) == ws(200, 2, -1, 3) == ws(200, 2, 10, -1) == ws(0, 2, 10, 3) == 0
    one, none = 8, None      # (a pointer that is never read: every call below returns before a launch)
    args = dict(loc=one, scale=one, pairs=one, match=none, ws=none, d_match=one, less=one, equal=one, nn_d=one, nn_idx=one, N=100,
                D=8, S=2, P=2, metric=0, keep=4, chunks=0, stream=none)
    for change, rc in ((dict(N=0), hipops.ERR_UNSUPPORTED), (dict(N=16385), hipops.ERR_UNSUPPORTED),
                       (dict(D=0), hipops.ERR_UNSUPPORTED), (dict(D=257), hipops.ERR_UNSUPPORTED),
                       (dict(S=1), hipops.ERR_UNSUPPORTED), (dict(S=17), hipops.ERR_UNSUPPORTED),
                       (dict(P=0), hipops.ERR_UNSUPPORTED), (dict(P=241), hipops.ERR_UNSUPPORTED),
                       (dict(keep=17), hipops.ERR_UNSUPPORTED), (dict(keep=-1), hipops.ERR_UNSUPPORTED),
                       (dict(metric=4), hipops.ERR_UNSUPPORTED), (dict(metric=-1), hipops.ERR_UNSUPPORTED),
                       (dict(chunks=-1), hipops.ERR_UNSUPPORTED), (dict(loc=none), hipops.ERR_ARG),
                       (dict(pairs=none), hipops.ERR_ARG), (dict(less=none), hipops.ERR_ARG), (dict(nn_idx=none), hipops.ERR_ARG),
                       (dict(scale=none, metric=2), hipops.ERR_ARG), (dict(scale=none, metric=3), hipops.ERR_ARG),
                       (dict(chunks=2), hipops.ERR_ARG)):      # (two chunks without a workspace)
        assert L.mmvae_retrieval_ranks(*dict(args, **change).values()) == rc, change


def test_ops_refuse_before_a_launch():
    from multimodal_vae_comparison_amd import ops
    loc, scale = torch.zeros(2, 6, 4), torch.ones(2, 6, 4)
    cases = [
        ("metric = 'l1'", (loc,), {"metric": "l1"}),
        ("keep = 17", (loc,), {"keep": 17}), ("keep = -1", (loc,), {"keep": -1}), ("chunks = -1", (loc,), {"chunks": -1}),
        ("loc is .*floating", (loc.long(),), {}), ("loc is .*floating", (loc[0],), {}),
        ("1 sets of", (loc[:1],), {}), ("17 sets of", (torch.zeros(17, 2, 2),), {}),
        ("sets of 16385 x 1", (torch.zeros(1, 1, 1).expand(2, 16385, 1),), {}),
        ("sets of 0 x 4", (torch.zeros(2, 0, 4),), {}), ("sets of 1 x 257", (torch.zeros(2, 1, 257),), {}),
        ("loc holds values that are not finite", (torch.full((2, 6, 4), float("nan")),), {}),
        ("'w2' compares distributions and needs `scale`", (loc,), {"metric": "w2"}),
        ("'skl' compares distributions and needs `scale`", (loc,), {"metric": "skl"}),
        (r"scale is \(2, 6, 3\)", (loc, torch.ones(2, 6, 3)), {"metric": "skl"}),
        ("scale holds values that are not positive", (loc, scale * 0), {"metric": "w2"}),
        ("scale holds values that are not finite", (loc, scale * float("inf")), {"metric": "w2"}),
        (r"pairs is \(1, 3\)", (loc,), {"pairs": [[0, 1, 0]]}), (r"pairs is \(241, 2\)", (loc,), {"pairs": [[0, 1]] * 241}),
        ("pairs is .*float", (loc,), {"pairs": torch.tensor([[0.0, 1.0]])}),
        ("two different sets out of 0 .. 1", (loc,), {"pairs": [[0, 0]]}),
        ("two different sets out of 0 .. 1", (loc,), {"pairs": [[0, 2]]}),
        ("two different sets out of 0 .. 1", (loc,), {"pairs": [[-1, 1]]}),
        (r"match is \(5,\)", (loc,), {"match": torch.arange(5)}), ("match is .*float", (loc,), {"match": torch.zeros(6)}),
        ("match holds entries outside -1 .. 5", (loc,), {"match": torch.tensor([0, 1, 2, 3, 4, 6])}),
        ("match holds entries outside -1 .. 5", (loc,), {"match": torch.tensor([0, 1, 2, 3, 4, -2])}),
        ("there is no host path", (loc,), {}), ("there is no host path", (loc, scale), {"metric": "skl", "keep": 16}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="retrieval_ranks: .*" + match):
            ops.retrieval_ranks(*args, **kwargs)
    assert ops.retrieval_pairs(3) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)] and len(ops.retrieval_pairs(16)) == 240


# ---- 4. the contract on CPU models --------------------------------------------------------------------------------------------------
def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


def test_unimodal_vae_refuses_cross_modal_retrieval_by_name():
    from multimodal_vae_comparison_amd.models.vae import MIXER_METRICS, VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE) and "cross_modal_retrieval" in MIXER_METRICS
    with pytest.raises(NotImplementedError) as e:
        vae.cross_modal_retrieval()
    assert "unimodal" in str(e.value) and "TorchMMVAE.cross_modal_retrieval" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="cross_modal_retrieval needs eval mode"):
        model.cross_modal_retrieval([cdsprites_batch(4, 6, seed=3)])


def test_argument_errors_come_before_the_first_encoder_call(monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    calls = []
    monkeypatch.setattr(model, "_sample", lambda *a, **kw: calls.append(1))
    monkeypatch.setattr(model, "latents_for", lambda *a, **kw: calls.append(1))
    half = dict(batch, mod_2=dict(batch["mod_2"], data=None))
    cases = [
        ("`batches` is empty", ([],), {}),
        ("metric = 'l1'", ([batch],), {"metric": "l1"}), ("use = 'prior'", ([batch],), {"use": "prior"}),
        ("samples are compared by 'l2' or 'cosine'", ([batch],), {"use": "sample", "metric": "skl"}),
        ("`given` selects the sets of use='sample'", ([batch],), {"given": [["mod_1"], ["mod_2"]]}),
        ("every batch must hold every modality", ([batch, half],), {}),
        ("names a modality without data", ([half],), {"use": "sample"}),
        ("must name modalities", ([batch],), {"use": "sample", "given": [["mod_1"], ["mod_9"]]}),
        ("must name modalities", ([batch],), {"use": "sample", "given": [["mod_1"], []]}),
        ("2 .. 16 different sets", ([batch],), {"use": "sample", "given": [["mod_1"]]}),
        ("2 .. 16 different sets", ([batch],), {"use": "sample", "given": [["mod_1"], ["mod_1"]]}),
        ("keep = 17", ([batch],), {"keep": 17}), ("ks = \\[\\]", ([batch],), {"ks": ()}), ("ks = \\[0\\]", ([batch],), {"ks": (0,)}),
        ("labels must be an integer", ([batch],), {"labels": torch.zeros(4)}),
        (r"labels is \(3, 1\), the batches hold 4 rows", ([batch],), {"labels": torch.tensor([0, 1, 0])}),
        ("negative values", ([batch],), {"labels": torch.tensor([0, 1, -1, 0])}),
        ("k <= keep nearest rows", ([batch],), {"labels": torch.tensor([0, 1, 1, 0]), "ks": (5,), "keep": 2}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="cross_modal_retrieval: .*" + match):
            model.cross_modal_retrieval(*args, **kwargs)
    big = dict(batch, mod_1=dict(batch["mod_1"], data=torch.zeros(1, 3, 64, 64).expand(16385, 3, 64, 64)))
    with pytest.raises(ValueError, match="cross_modal_retrieval: 16385 rows .*MI355X path"):
        model.cross_modal_retrieval([big])
    assert not calls and model._eval_draws is False and model.eps_override is None


def test_a_failing_call_leaves_the_noise_setup_as_it_found_it():
    """on a CPU model the first encoder call fails inside the noise context"""
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    mine = model.eps_override = [torch.zeros(4, 8)]

    def broken(*a, **kw):
        assert model._eval_draws is True and not torch.is_grad_enabled()
        raise KeyError("the encoders fail inside the noise context")

    model._sample = broken
    for use in ("posterior", "sample"):
        with pytest.raises(KeyError):
            model.cross_modal_retrieval([batch], use=use)
        assert model._eval_draws is False and torch.is_grad_enabled()
        assert model.eps_override is mine and len(mine) == 1


def test_trainer_wrapper_logs_per_pair(monkeypatch):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods("poe", CD_MODS, 8, batch_size=4)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cpu")
    fake = {"mod_1->mod_2": {"recall@1": 0.5, "recall@5": 1.0, "median_rank": 1.5, "mrr": 0.75, "mean_rank": 2.0, "n": 4,
                             "d_match": torch.zeros(4)}, "mean": {"recall@1": 0.5}}
    monkeypatch.setattr(tr.model, "cross_modal_retrieval", lambda batches, **kw: fake)
    logged = {}
    monkeypatch.setattr(tr, "log", lambda name, v, **kw: logged.__setitem__(name, float(v)))
    assert tr.cross_modal_retrieval([None], metric="cosine") is fake
    assert logged == {"test_retrieval_recall@1_mod_1->mod_2": 0.5, "test_retrieval_recall@5_mod_1->mod_2": 1.0,
                      "test_retrieval_median_rank_mod_1->mod_2": 1.5, "test_retrieval_mrr_mod_1->mod_2": 0.75}
