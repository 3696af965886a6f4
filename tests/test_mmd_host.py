"""Host tests of the kernel two-sample test (csrc/mmd.hip): the numpy restatement of
tests/mmd_reference.py against a plain double loop, against torch and against a case worked by hand; the identities the
kernel's route rests on; the recipe of ops.mmd_draw; the automatic width; the separation of the permuted estimates from
the observed one that lets the GPU tests compare p-values exactly; the ABI; every refusal before a launch; and seeded
errors in the restatement, each failing exactly its part."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mmd_reference as R
from conftest import ROOT

SYMBOLS = ("mmvae_mmd_chunks", "mmvae_mmd_ws_doubles", "mmvae_mmd_sums")


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------
def loop_sums(X, Y, member, kernel, params):
    """the three sums of every split and the row sums by a plain double loop over the pairs"""
    Z = np.concatenate([X, Y]).astype(np.float64)
    n, A = len(Z), R.splits(len(X), len(Y), member)
    sums, rows = np.zeros((len(A), 3)), np.zeros(n)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            d2 = float(np.sum((Z[i] - Z[j]) ** 2))
            if kernel == "energy":
                k = -np.sqrt(d2)
            else:
                k = sum(np.exp(-p * d2) if kernel == "rbf" else p / (p + d2) for p in params) / len(params)
            rows[i] += k
            for s, a in enumerate(A):
                sums[s, 0 if a[i] and a[j] else 1 if not a[i] and not a[j] else 2] += k if a[i] == a[j] else 0.5 * k
    return sums, rows


@pytest.mark.parametrize("name", ["2x2", "dup-rbf", "dup-imq", "dup-energy", "far"])
def test_restatement_against_a_plain_loop(name):
    c = R.case(name)
    sums, rows = loop_sums(c.X, c.Y, c.member, c.kernel, c.params)
    scale = c.ld["abs_sums"].astype(np.float64)
    assert np.all(np.abs(sums - c.f64["sums"]) <= 1e-12 * scale) and np.all(np.abs(sums - c.ld["sums"]) <= 1e-12 * scale)
    assert np.all(np.abs(rows - c.f64["row_sums"]) <= 1e-12 * c.ld["abs_rows"].astype(np.float64))


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_against_torch(name):
    """cdist in float64, the kernel function and (A @ K * A).sum(1): the composed route of tools/bench_mmd.py"""
    c = R.case(name)
    Z = torch.from_numpy(np.concatenate([c.X, c.Y])).double()
    d2 = torch.cdist(Z, Z, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    if c.kernel == "energy":
        K = -d2.sqrt()
    else:
        K = sum(torch.exp(-p * d2) if c.kernel == "rbf" else p / (p + d2) for p in c.params) / len(c.params)
    K.fill_diagonal_(0.0)
    A = torch.from_numpy(R.splits(c.n_x, c.n_y, c.member)).double()
    B = 1 - A
    got = torch.stack([(A @ K * A).sum(1), (B @ K * B).sum(1), (A @ K * B).sum(1)], 1).numpy()
    # cdist takes a root and the test squares it again: a few roundings per term more than the restatement's own
    assert np.all(np.abs(got - c.f64["sums"]) <= 1e-11 * c.ld["abs_sums"].astype(np.float64)), name
    assert np.all(np.abs(K.sum(1).numpy() - c.f64["row_sums"]) <= 1e-11 * c.ld["abs_rows"].astype(np.float64))


@pytest.mark.parametrize("name", R.NAMES)
def test_identities(name):
    """with r = K 1, T = 1' r, l = a' r and q = a' K a: sum over Y = T - 2 l + q, cross = l - q, and the three sums (the
    cross sum twice) add up to T -- in longdouble, to its rounding"""
    c = R.case(name)
    K, A = c.ld["K"], R.splits(c.n_x, c.n_y, c.member).astype(R.LD)
    r = K.sum(1)
    T, l, q = r.sum(), A @ r, ((A @ K) * A).sum(1)
    s, tol = c.ld["sums"], 64 * np.finfo(R.LD).eps * np.abs(K).sum()
    assert np.all(np.abs(s[:, 0] - q) <= tol) and np.all(np.abs(s[:, 1] - (T - 2 * l + q)) <= tol)
    assert np.all(np.abs(s[:, 2] - (l - q)) <= tol) and np.all(np.abs(s[:, 0] + s[:, 1] + 2 * s[:, 2] - T) <= tol)
    assert np.all(np.abs(r - c.ld["row_sums"]) == 0) and np.all(K == K.T) and np.all(np.diag(K) == 0)
    assert np.all(c.bound["sums"] >= R.FLOOR * c.ld["abs_sums"].astype(np.float64))
    assert np.all(c.bound["sums"] >= R.FACTOR * c.err["sums"]) and c.ld["sums"].shape == (1 + c.P, 3)


def test_integer_case_by_hand():
    """X = {0, 1}, Y = {3, 6} on a line, energy kernel k = -d: pooled distances 1, 3, 6, 2, 5, 3"""
    X, Y = np.array([[0.0], [1.0]], np.float32), np.array([[3.0], [6.0]], np.float32)
    member = np.array([[1, 0, 1, 0], [0, 1, 1, 0]], np.uint8)      # {0, 3} | {1, 6} and {1, 3} | {0, 6}
    for dtype in (np.float64, R.LD):
        out = R.restate(X, Y, member, "energy", (), dtype)
        assert out["sums"].tolist() == [[-2.0, -6.0, -16.0], [-6.0, -10.0, -12.0], [-4.0, -12.0, -12.0]]
        assert out["row_sums"].tolist() == [-10.0, -8.0, -8.0, -14.0]
        est = R.mmd2_of(out["sums"], 2, 2)
        assert est.tolist() == [4.0, -2.0, -2.0]      # (-2 - 6) / 2 + 16 / 2;   (-6 - 10) / 2 + 12 / 2;   (-4 - 12) / 2 + 6
    assert R.p_value(4.0, [-2.0, -2.0]) == 1 / 3 and R.p_value(-2.0, [4.0, -2.0]) == 1.0 and R.p_value(1.0, []) == 1.0
    # a Gaussian kernel of rate ln 2: k = 2^(-d^2), exact in binary
    out = R.restate(X, Y, None, "rbf", (np.log(2.0),), np.float64)
    assert np.allclose(out["sums"], [[2 * 0.5, 2 * 2.0 ** -9, 2.0 ** -9 + 2.0 ** -36 + 2.0 ** -4 + 2.0 ** -25]], rtol=1e-15)


def test_draw_is_the_documented_recipe():
    from multimodal_vae_comparison_amd import ops
    for n_x, n_y, P, seed in ((5, 7, 4, 0), (2, 2, 3, 7), (64, 65, 9, 123), (3, 4, 0, 1)):
        got = ops.mmd_draw(n_x, n_y, P, seed)
        rs = np.random.RandomState(seed)
        want = np.zeros((P, n_x + n_y), np.uint8)
        for p in range(P):
            want[p, rs.permutation(n_x + n_y)[:n_x]] = 1
        assert got.dtype == np.uint8 and got.shape == (P, n_x + n_y) and np.array_equal(got, want)
        assert np.array_equal(got, R.draw(n_x, n_y, P, seed)) and np.all(got.sum(1) == n_x)
    assert "rs.permutation" in ops.mmd_draw.__doc__ and "RandomState(seed)" in ops.mmd_draw.__doc__


def test_automatic_width_is_the_mean_squared_distance():
    for name in ("2x2", "n129-D1-S8", "offset-rbf", "n193-D256"):
        c = R.case(name)
        d2 = R.sqdist(np.concatenate([c.X, c.Y]), R.LD)
        m2 = float(d2.sum() / (c.n * (c.n - 1)))      # (the diagonal holds zeros)
        for kernel in ("rbf", "imq"):
            params = R.auto_params(np.concatenate([c.X, c.Y]), kernel, c.scales)
            want = [1.0 / (s * m2) if kernel == "rbf" else s * m2 for s in c.scales]
            # (offset: the variance of rows near 1000 in float64 keeps nine digits of m2)
            assert np.allclose(params, want, rtol=1e-8 if name.startswith("offset") else 1e-12, atol=0.0), (name, kernel)
    assert R.auto_params(np.zeros((4, 2)), "energy") == ()


# ---- 2. what lets the p-values be compared exactly ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_no_permuted_estimate_lies_near_the_observed_one(name):
    """an estimate may move by its bound; the count behind the p-value cannot change while every permuted estimate stays
    1000 bounds away from the observed one"""
    c = R.case(name)
    assert c.apart() > 1.0, (name, c.apart())
    print(f"{name}: nearest permuted estimate {c.apart():.3g} x 1000 bounds away; p = {c.p_value}")
    f64 = R.mmd2_of(c.f64["sums"], c.n_x, c.n_y)
    assert R.p_value(f64[0], f64[1:]) == c.p_value


def test_same_and_shifted_on_the_reference():
    same, shifted = R.case("same"), R.case("shifted")
    assert same.p_value > 0.05 and shifted.p_value == 1.0 / (1 + shifted.P) and same.P == shifted.P == 199


def test_the_case_table_covers_the_edges():
    from multimodal_vae_comparison_amd import hipops as H
    assert (R.PBLOCK, R.EXTRA, R.SCALES) == (H.MMD_PBLOCK, H.MMD_EXTRA_COLUMNS, (0.25, 0.5, 1.0, 2.0, 4.0))
    cases = [R.CASES[n] for n in R.NAMES]
    assert {(c[1], c[2]) for c in cases} >= {(2, 2), (63, 65), (64, 64), (65, 128)}
    assert {c[1] + c[2] for c in cases} >= {127, 129, 191, 193, 255, 257} and max(c[1] + c[2] for c in cases) == 300
    assert {c[3] for c in cases} >= {1, 31, 32, 33, 256}
    border = H.MMD_PBLOCK - H.MMD_EXTRA_COLUMNS      # relabellings that fill the first block of columns
    assert {c[4] for c in cases} >= {0, 1, border - 1, border, border + 1}
    assert {len(c[7]) for c in cases if c[7]} >= {1, 5, 8} and {c[5] for c in cases} == {"rbf", "imq", "energy"}
    assert {c[0] for c in cases} == set(R.DATA)
    c = R.case("far")
    K = c.ld["K"].astype(np.float64)
    assert np.mean(K[~np.eye(c.n, dtype=bool)] == 0.0) > 0.45      # (the terms between the clusters underflow)
    off = R.case("offset-rbf")
    assert off.X.dtype == np.float32 and abs(float(off.X.mean()) - 1000.0) < 0.01 and 0.005 < float(off.X.std()) < 0.02


# ---- 3. the ABI --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_limits():
    from multimodal_vae_comparison_amd import hipops, ops
    from multimodal_vae_comparison_amd.models.vae import MIXER_METRICS
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES, f"{name} is not in the ctypes table"
        assert hasattr(hipops.lib(), name)
    for macro, value in (("MMVAE_MMD_MAX_ROWS", hipops.MMD_MAX_ROWS), ("MMVAE_MMD_MAX_D", hipops.MMD_MAX_D),
                         ("MMVAE_MMD_MAX_PERMUTATIONS", hipops.MMD_MAX_PERMUTATIONS),
                         ("MMVAE_MMD_MAX_SCALES", hipops.MMD_MAX_SCALES), ("MMVAE_MMD_PBLOCK", hipops.MMD_PBLOCK),
                         ("MMVAE_MMD_RBF", hipops.MMD_KERNELS["rbf"]), ("MMVAE_MMD_IMQ", hipops.MMD_KERNELS["imq"]),
                         ("MMVAE_MMD_ENERGY", hipops.MMD_KERNELS["energy"])):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value, macro
    assert (hipops.MMD_MAX_ROWS, hipops.MMD_MAX_D, hipops.MMD_MAX_PERMUTATIONS, hipops.MMD_MAX_SCALES) == (16384, 256, 2048, 8)
    assert "latent_two_sample" in MIXER_METRICS
    assert "mmd.hip" in open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "Makefile")).read()
    for name in ("mmd_sums", "mmd_draw", "mmd_two_sample"):
        assert callable(getattr(ops, name))
    tail = open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "ops.py")).read().rstrip().splitlines()[-1]
    assert tail.startswith("from .metrics.mmd import *")


def test_pure_queries_and_refusals_of_the_entry_point_run_without_gpu():
    from multimodal_vae_comparison_amd import hipops as H
    L = H.lib()
    chunks, ws = L.mmvae_mmd_chunks, L.mmvae_mmd_ws_doubles
    # min(ceil(512 / tiles), ceil(tiles / 4)) chunks, tiles = ceil(n / 64): a function of n alone
    assert [chunks(n) for n in (4, 64, 256, 257, 300, 1024, 10000, 16384)] == [1, 1, 1, 2, 2, 4, 4, 2]
    assert chunks(3) == chunks(16385) == chunks(0) == 0
    assert ws(3, 8, 10, 0) == ws(16385, 8, 10, 0) == ws(100, 0, 10, 0) == ws(100, 257, 10, 0) == 0
    assert ws(100, 8, -1, 0) == ws(100, 8, 2049, 0) == ws(100, 8, 10, -1) == 0

    def doubles(n, D, P, c):
        even = lambda v: v + (v & 1)
        tiles, pc = -(-n // 64), -(-(P + H.MMD_EXTRA_COLUMNS) // H.MMD_PBLOCK) * H.MMD_PBLOCK
        return 8 + even(D) + even(n) + even(n * D) + even(c * n) + 2 * tiles * c * pc + 8 * tiles * pc
    assert ws(300, 8, 20, 0) == doubles(300, 8, 20, 2) and ws(300, 8, 20, 5) == doubles(300, 8, 20, 5)
    assert ws(300, 8, 20, 9) == doubles(300, 8, 20, 5) and ws(129, 1, 127, 0) == doubles(129, 1, 127, 1)
    assert ws(129, 1, 128, 1) == doubles(129, 1, 128, 1) > ws(129, 1, 127, 1)
    assert ws(16384, 256, 2048, 0) == doubles(16384, 256, 2048, 2)
    # refusals come before any launch: no device pointer is read
    buf = (ctypes.c_double * 64)()
    p, prm = ctypes.cast(buf, H.c_p), (ctypes.c_double * 8)(*([1.0] * 8))
    base = dict(X=p, Y=p, member=p, ws=p, sums=p, row_sums=p, n_x=8, n_y=8, D=4, P=2, family=0, params=ctypes.cast(prm, H.c_p),
                S=2, chunks=0, stream=None)

    def call(**k):
        return L.mmvae_mmd_sums(*{**base, **k}.values())
    for bad in (dict(n_x=1), dict(n_y=1), dict(n_x=16383), dict(n_x=20000), dict(D=0), dict(D=257), dict(P=-1), dict(P=2049),
                dict(S=0), dict(S=9), dict(family=3), dict(family=-1), dict(chunks=-1)):
        assert call(**bad) == H.ERR_UNSUPPORTED, bad
    for bad in (dict(X=None), dict(Y=None), dict(member=None), dict(ws=None), dict(sums=None), dict(row_sums=None),
                dict(params=None)):
        assert call(**bad) == H.ERR_ARG, bad
    for value in (0.0, -1.0, float("inf"), float("nan")):
        prm[1] = value
        assert call() == H.ERR_ARG, value


# ---- 4. the refusals of the wrappers and of the model ---------------------------------------------------------------------------------
def test_every_operand_refusal_comes_before_a_launch():
    from multimodal_vae_comparison_amd import hipops as H, ops
    x, y = torch.randn(6, 3), torch.randn(5, 3)
    member = torch.from_numpy(R.draw(6, 5, 2, 0))
    calls = H.CALLS[0]
    cases = [
        ("X is .*floating", (x.long(), y), {}), ("Y is .*floating", (x, y[0]), {}), ("X has 1 rows", (x[:1], y), {}),
        ("Y has 1 rows", (x, y[:1]), {}), ("X has D = 257", (torch.randn(4, 257), torch.randn(4, 257)), {}),
        ("X has 16385 rows", (torch.zeros(1, 3).expand(16385, 3), y), {}),
        ("16380 \\+ 5 = 16385 rows together", (torch.zeros(1, 3).expand(16380, 3), y), {}),
        ("X has D = 3 dimensions, Y D = 2", (x, y[:, :2]), {}),
        ("X holds values that are not finite", (x * float("inf"), y), {}),
        ("Y holds values that are not finite", (x, torch.full((5, 3), float("nan"))), {}),
        ("kernel = 'poly'", (x, y), {"kernel": "poly"}), ("chunks = -1", (x, y), {"chunks": -1}),
        ("params = \\(\\)", (x, y), {"params": ()}), ("params = \\(1.0, -2.0\\)", (x, y), {"params": (1.0, -2.0)}),
        ("params = \\(nan,\\)", (x, y), {"params": (float("nan"),)}), ("params is int", (x, y), {"params": 3}),
        ("params = ", (x, y), {"params": [1.0] * 9}), ("scales = \\(0.0,\\)", (x, y), {"scales": (0.0,)}),
        ("scales = ", (x, y), {"scales": [1.0] * 9, "kernel": "imq"}),
        ("energy kernel k = -d has no parameters", (x, y), {"kernel": "energy", "params": (1.0,)}),
        ("member is .*integer", (x, y, member.float()), {}), ("member is .*integer", (x, y, member[0]), {}),
        ("member is 2 relabellings of 10 pooled rows", (x, y, member[:, :10]), {}),
        ("member is 2049 relabellings", (x, y, torch.zeros(2049, 11, dtype=torch.uint8)), {}),
        ("values from 0 to 3", (x, y, member * 3), {}), ("values from -1 to 1", (x, y, torch.where(member.bool(), 1, -1)), {}),
        ("mark 5 .. 6 pooled rows", (x, y, torch.cat([member[:1], 1 - member[:1]])), {}),
        ("mean squared distance of the pooled rows is 0.0", (torch.ones(3, 2), torch.ones(4, 2)), {}),
        ("X is on cpu; the kernel runs on the MI355X", (x, y, member), {}),
        ("X is on cpu", (x, y), {"kernel": "energy"}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="mmd_sums: .*" + match):
            ops.mmd_sums(*args, **kwargs)
    for match, args, kwargs in [("permutations = 2049", (x, y), {"permutations": 2049}),
                                ("permutations = -1", (x, y), {"permutations": -1}),
                                ("X and Y are floating", (x, None), {}), ("X has 1 rows", (x[:1], y), {}),
                                ("X is on cpu", (x, y), {"permutations": 3})]:
        with pytest.raises(ValueError, match="mmd_two_sample: .*" + match):
            ops.mmd_two_sample(*args, **kwargs)
    assert H.CALLS[0] == calls, "a refusal came after a C call"


def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


def test_unimodal_vae_refuses_latent_two_sample_by_name():
    from multimodal_vae_comparison_amd.models.vae import MIXER_METRICS, VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE) and "latent_two_sample" in MIXER_METRICS
    with pytest.raises(NotImplementedError) as e:
        vae.latent_two_sample()
    assert "unimodal" in str(e.value) and "TorchMMVAE.latent_two_sample" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="latent_two_sample needs eval mode"):
        model.latent_two_sample([cdsprites_batch(4, 6, seed=3)])


def test_argument_errors_come_before_the_first_encoder_call(monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    calls = []
    monkeypatch.setattr(model, "_sample", lambda *a, **kw: calls.append(1))
    monkeypatch.setattr(model, "latents_for", lambda *a, **kw: calls.append(1))
    half = dict(batch, mod_2=dict(batch["mod_2"], data=None))
    three = dict(batch, mod_1=dict(batch["mod_1"], data=batch["mod_1"]["data"][:3]))
    big = dict(batch, mod_1=dict(batch["mod_1"], data=torch.zeros(1, 3, 64, 64).expand(8193, 3, 64, 64)))
    cases = [
        ("`batches` is empty", ([],), {}), ("kernel = 'poly'", ([batch],), {"kernel": "poly"}),
        ("permutations = 2049", ([batch],), {"permutations": 2049}), ("permutations = -1", ([batch],), {"permutations": -1}),
        ("must name modalities", ([batch],), {"given": [["mod_1"], ["mod_9"]]}),
        ("must name modalities", ([batch],), {"given": [["mod_1"], []]}),
        ("different conditioning subsets", ([batch],), {"given": [["mod_1"], ["mod_1"]]}),
        ("names a modality without data", ([half],), {}), ("3 rows of 8 latent dimensions", ([three],), {"given": [["mod_1"]]}),
        ("8193 rows of 8 latent dimensions", ([big],), {"given": [["mod_1"]]}),
        ("density is a result of fit_latent_density", ([batch],), {"density": {"mod_3": {}}}),
        ("density is a result of fit_latent_density", ([batch],), {"density": 3}),
        (r"eps is \(4, 7\)", ([batch],), {"eps": torch.zeros(4, 7)}), ("eps is int", ([batch],), {"eps": 1}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="latent_two_sample: .*" + match):
            model.latent_two_sample(*args, **kwargs)
    assert not calls
    doc = type(model).latent_two_sample.__doc__
    assert "EVEN rows" in doc and "ODD rows" in doc and "independent" in doc


# ---- 5. seeded errors: each fails exactly its part -----------------------------------------------------------------------------------
def _fails(c, out, n_x=None, n_y=None, divisor_bug=False):
    """which parts a wrong restatement gets wrong, against the right one's bounds: (sums, row sums, estimate)"""
    es = np.abs(out["sums"] - c.ld["sums"]).astype(np.float64) > c.bound["sums"]
    er = np.abs(out["row_sums"] - c.ld["row_sums"]).astype(np.float64) > c.bound["row_sums"]
    est = R.mmd2_of(out["sums"], c.n_x, c.n_y, divisor_bug=divisor_bug)
    ee = np.abs(est - c.mmd2).astype(np.float64) > 2.0 * c.mmd2_bound
    return es, er, ee


@pytest.mark.parametrize("name", ["n300-D8", "shifted", "n255-D5-energy", "n257-D40-imq-S8"])
def test_seeded_errors(name):
    c = R.case(name)
    right = R.restate(c.X, c.Y, c.member, c.kernel, c.params, R.LD)
    assert not any(part.any() for part in _fails(c, right))
    # the diagonal kept: the within-set sums and every row sum move (k(0) = 1), the cross sum does not; the energy kernel
    # has k(0) = 0 and cannot tell
    es, er, _ = _fails(c, R.restate(c.X, c.Y, c.member, c.kernel, c.params, R.LD, keep_diagonal=True))
    if c.kernel == "energy":
        assert not es.any() and not er.any()
    else:
        assert es[:, :2].all() and not es[:, 2].any() and er.all()
    # the wrong divisor: the sums are right, every estimate is wrong
    es, er, ee = _fails(c, right, divisor_bug=True)
    assert not es.any() and not er.any() and ee.all()
    # the groups swapped: sxx and syy change places (different sizes or different sets: they differ), the cross sum and the
    # row sums stay
    es, er, _ = _fails(c, R.restate(c.X, c.Y, c.member, c.kernel, c.params, R.LD, swap=True))
    assert es[:, :2].all() and not es[:, 2].any() and not er.any()
    # gamma applied to d instead of d^2: every sum and row sum of a family with a width moves; k = -d has none
    if c.kernel != "energy":
        es, er, _ = _fails(c, R.restate(c.X, c.Y, c.member, c.kernel, c.params, R.LD, root_in_rbf=True))
        assert es.all() and er.all()
