"""Host checks of the image reconstruction quality.  The float64 restatement the GPU tests of
csrc/image_quality.hip are held to (tests/image_quality_reference.py: direct 2-D window sums) against an independent route --
scipy.ndimage's separable filters over the whole plane, cropped by (win - 1) / 2, the route scikit-image takes -- and against
closed forms; the ABI of the new entry points and their pure queries; reconstruction_quality keeps the metrics' contract on CPU
models, where nothing reaches a kernel; ops.image_quality refuses what is outside the limits before any device call."""
import math
import os
import re

import numpy as np
import pytest
import scipy.ndimage
import torch

import image_quality_reference as R
from conftest import ROOT

SYMBOLS = ("mmvae_image_quality", "mmvae_image_quality_max_scales", "mmvae_image_quality_lds_bytes")


# ---- 1. the restatement against the separable route ----------------------------------------------------------------------------
def _scipy_levels(x, y, win, sigma, data_range, k1, k2, sample_covariance, scales):
    """scikit-image's route: filter the whole plane (scipy.ndimage, separable), crop by (win - 1) / 2 -> per level the images'
    (ssim, cs, l)"""
    x, y, pad = x.astype(np.float64), y.astype(np.float64), (win - 1) // 2
    if sigma is None:
        def filt(t):
            return scipy.ndimage.uniform_filter(t, size=(1, 1, win, win), mode="constant")
    else:
        i = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
        g = np.exp(-(i * i) / (2.0 * sigma * sigma))
        g /= g.sum()

        def filt(t):
            t = scipy.ndimage.correlate1d(t, g, axis=2, mode="constant")
            return scipy.ndimage.correlate1d(t, g, axis=3, mode="constant")
    f = win * win / (win * win - 1.0) if sample_covariance else 1.0
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    out = []
    for s in range(scales):
        mx, my, xx, yy, xy = (filt(t)[:, :, pad:t.shape[2] - pad, pad:t.shape[3] - pad] for t in (x, y, x * x, y * y, x * y))
        vx, vy, cxy = f * (xx - mx * mx), f * (yy - my * my), f * (xy - mx * my)
        l, cs = (2 * mx * my + c1) / (mx * mx + my * my + c1), (2 * cxy + c2) / (vx + vy + c2)
        out.append(tuple(t.mean((2, 3)).mean(1) for t in (l * cs, cs, l)))
        if s + 1 < scales:
            x, y = R.pool(x), R.pool(y)
    return out


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_restatement_against_the_separable_route(i):
    x, y, kw, ref = R.case(i)
    full = dict(win=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, sample_covariance=False, scales=1)
    full.update(kw)
    given = full.pop("weights", None)
    S = full["scales"]
    other = _scipy_levels(x, y, **full)
    bar = ref["bar"]
    e = np.abs(other[0][0] - ref["ssim"]) / bar["ssim"]
    print(f"{R.IDS[i]}: ssim of the two routes {e.max():.3g} bars (bar {bar['ssim'].max():.3g})")
    assert e.max() <= 1.0
    for s in range(S):
        e = np.abs(other[s][1 if s + 1 < S else 2] - ref["levels"][:, s]) / bar["levels"][:, s]
        print(f"  level {s + 1}: {e.max():.3g} bars")
        assert e.max() <= 1.0
    assert ref["levels"].shape == (x.shape[0], S)
    # the bound never exceeds the flat ceiling 12 f gamma (1 / C1 + 1 / C2) (both denominators are at least their constant)
    L, f = full["data_range"], (full["win"] ** 2 / (full["win"] ** 2 - 1.0) if full["sample_covariance"] else 1.0)
    ceiling = 12 * f * (full["win"] ** 2 + 8) * R.U * L * L * (1 / (0.01 * L) ** 2 + 1 / (0.03 * L) ** 2)
    assert np.all(bar["ssim"] <= 4 * ceiling * (1 + 1e-9)) and np.all(bar["levels"] <= 4 * ceiling * (1 + 1e-9))
    # psnr and the errors from their definitions, element by element in another order
    d = x.astype(np.float64).reshape(len(x), -1) - y.astype(np.float64).reshape(len(x), -1)
    mse = np.array([math.fsum(v * v for v in row) / len(row) for row in d[:4]])
    mae = np.array([math.fsum(abs(v) for v in row) / len(row) for row in d[:4]])
    assert np.all(np.abs(mse - ref["mse"][:4]) <= bar["mse"][:4]) and np.all(np.abs(mae - ref["mae"][:4]) <= bar["mae"][:4])
    L = full["data_range"]
    assert np.all(np.abs(10 * np.log10(L * L / mse) - ref["psnr"][:4]) <= bar["psnr"][:4])
    if S > 1:
        assert ref["values"].min() >= 0.05
        w = np.asarray(R.MS_WEIGHTS[:S]) / sum(R.MS_WEIGHTS[:S]) if given is None else np.asarray(given)
        want = np.prod([np.maximum(other[s][1 if s + 1 < S else 2], 0.0) ** w[s] for s in range(S)], axis=0)
        assert np.all(np.abs(want - ref["ms_ssim"]) <= bar["ms_ssim"])


def test_window_and_weights():
    from multimodal_vae_comparison_amd import ops
    for win, sigma in ((11, 1.5), (7, None), (3, 0.5), (5, 2.0)):
        g = ops.image_quality_window(win, sigma)
        assert g.dtype == np.float64 and g.shape == (win,) and abs(g.sum() - 1.0) <= 4 * R.U
        assert np.abs(np.outer(g, g) - R.window(win, sigma)).max() <= 8 * R.U
    assert ops.MS_SSIM_WEIGHTS == R.MS_WEIGHTS
    plan = ops.image_quality_plan((2, 3, 64, 64), scales=3)
    assert np.allclose(plan["weights"], np.asarray(R.MS_WEIGHTS[:3]) / sum(R.MS_WEIGHTS[:3]), rtol=0, atol=2 * R.U)
    assert plan["c1"] == 1e-4 and plan["c2"] == (0.03 * 1.0) ** 2 and plan["cov_scale"] == 1.0
    assert ops.image_quality_plan((2, 3, 28, 28), win=7, sigma=None, sample_covariance=True)["cov_scale"] == 49.0 / 48.0
    assert ops.image_quality_plan((1, 1, 64, 64), scales=2, weights=[0.25, 0.75])["weights"] == [0.25, 0.75]


# ---- 2. closed forms ------------------------------------------------------------------------------------------------------------------
def test_identical_images():
    x = np.random.RandomState(3).uniform(size=(3, 2, 20, 24)).astype(np.float32)
    r = R.image_quality(x, x, win=7, scales=2)
    assert np.all(r["mse"] == 0.0) and np.all(r["mae"] == 0.0) and np.all(np.isposinf(r["psnr"]))
    assert np.all(np.abs(r["ssim"] - 1.0) <= r["bar"]["ssim"]) and np.all(np.abs(r["levels"] - 1.0) <= r["bar"]["levels"])
    assert np.all(np.abs(r["ms_ssim"] - 1.0) <= r["bar"]["ms_ssim"])


def test_two_constant_planes():
    a, b = 0.3, 0.8
    x, y = np.full((1, 1, 16, 16), a, dtype=np.float32), np.full((1, 1, 16, 16), b, dtype=np.float32)
    a, b = float(x[0, 0, 0, 0]), float(y[0, 0, 0, 0])
    for kw in (dict(win=11), dict(win=5, sigma=None, sample_covariance=True), dict(win=7, data_range=2.0)):
        r = R.image_quality(x, y, scales=1, **kw)
        c1 = (0.01 * kw.get("data_range", 1.0)) ** 2
        want = (2 * a * b + c1) / (a * a + b * b + c1)
        assert abs(r["ssim"][0] - want) <= r["bar"]["ssim"][0] and abs(r["levels"][0, 0] - want) <= r["bar"]["levels"][0, 0]
        two = R.image_quality(x, y, scales=2, **dict(kw, win=min(kw["win"], 7)))
        assert abs(two["levels"][0, 0] - 1.0) <= two["bar"]["levels"][0, 0]      # cs of constant planes
        assert abs(r["mse"][0] - (a - b) ** 2) <= r["bar"]["mse"][0] and abs(r["mae"][0] - abs(a - b)) <= r["bar"]["mae"][0]


@pytest.mark.parametrize("win, sigma", [(11, 1.5), (7, None), (3, 1.0)])
def test_one_position_is_the_formula_on_the_global_moments(win, sigma):
    rs = np.random.RandomState(win)
    x, y = (rs.uniform(size=(1, 1, win, win)).astype(np.float32) for _ in range(2))
    r = R.image_quality(x, y, win=win, sigma=sigma)
    w = R.window(win, sigma)
    terms = [(float(w[i, j]), float(x[0, 0, i, j]), float(y[0, 0, i, j])) for i in range(win) for j in range(win)]
    mx, my = math.fsum(k * p for k, p, _ in terms), math.fsum(k * q for k, _, q in terms)
    vx = math.fsum(k * p * p for k, p, _ in terms) - mx * mx
    vy = math.fsum(k * q * q for k, _, q in terms) - my * my
    cxy = math.fsum(k * p * q for k, p, q in terms) - mx * my
    c1, c2 = 1e-4, 9e-4
    want_l, want_cs = (2 * mx * my + c1) / (mx * mx + my * my + c1), (2 * cxy + c2) / (vx + vy + c2)
    assert abs(r["ssim"][0] - want_l * want_cs) <= r["bar"]["ssim"][0]
    assert abs(r["levels"][0, 0] - want_l) <= r["bar"]["levels"][0, 0]
    assert r["ms_ssim"][0] == max(r["ssim"][0], 0.0)


def test_a_negative_is_anti_correlated():
    x, y = R.anti_correlated()
    r = R.image_quality(x, y, win=11, scales=2)
    assert np.all(r["levels"][:, 0] < -0.5), r["levels"]      # the mean cs of level 1
    assert np.all(r["ms_ssim"] == 0.0) and np.all(r["levels"][:, 1] > 0.5)
    one = R.image_quality(x, y, win=11)
    assert np.all(one["ssim"] < 0.0) and np.all(one["ms_ssim"] == 0.0)
    assert np.all(r["mse"] == 1.0) and np.all(r["psnr"] == 0.0)


# ---- 3. the ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from multimodal_vae_comparison_amd import hipops
    from multimodal_vae_comparison_amd.models.vae import MIXER_METRICS
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES, f"{name} is not in the ctypes table"
        assert hasattr(hipops.lib(), name)
    for macro, value in (("MMVAE_IQ_MIN_WIN", hipops.IQ_MIN_WIN), ("MMVAE_IQ_MAX_WIN", hipops.IQ_MAX_WIN),
                         ("MMVAE_IQ_MAX_SIDE", hipops.IQ_MAX_SIDE), ("MMVAE_IQ_MAX_CHANNELS", hipops.IQ_MAX_CHANNELS),
                         ("MMVAE_IQ_MAX_SCALES", hipops.IQ_MAX_SCALES), ("MMVAE_IQ_MAX_ROWS", hipops.IQ_MAX_ROWS)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value, macro
    assert "reconstruction_quality" in MIXER_METRICS
    assert "image_quality.hip" in open(os.path.join(ROOT, "multimodal_vae_comparison_amd", "csrc", "Makefile")).read()


def test_pure_queries_run_without_gpu():
    from multimodal_vae_comparison_amd import hipops
    L = hipops.lib()
    q = L.mmvae_image_quality_max_scales
    assert (q(64, 64, 11), q(28, 28, 11), q(32, 32, 11), q(64, 64, 3), q(64, 64, 7), q(11, 11, 11)) == (3, 2, 2, 4, 4, 1)
    assert (q(44, 44, 11), q(46, 44, 11), q(64, 22, 11), q(64, 24, 11), q(12, 17, 3)) == (3, 2, 2, 2, 1)
    assert (q(64, 64, 10), q(64, 64, 13), q(64, 64, 1), q(65, 64, 11), q(64, 65, 3), q(10, 64, 11), q(64, 10, 11)) == (0,) * 7
    b = L.mmvae_image_quality_lds_bytes
    assert b(64, 64, 11) == 81504 and b(33, 11, 11) == 81504 and b(32, 32, 11) == 31840 and b(28, 28, 7) < b(28, 28, 11)
    assert 2 * b(64, 64, 11) <= 160 * 1024 and b(64, 64, 12) == 0 and b(8, 8, 9) == 0
    # the plan of the op allows exactly what the query allows
    from multimodal_vae_comparison_amd import ops
    for H, W, win in ((64, 64, 11), (28, 28, 11), (46, 44, 11), (64, 64, 7), (12, 17, 3), (40, 64, 5)):
        top = q(H, W, win)
        assert ops.image_quality_plan((1, 1, H, W), win=win, scales=top)["scales"] == top
        with pytest.raises(ValueError, match="image_quality: "):
            ops.image_quality_plan((1, 1, H, W), win=win, scales=top + 1)


# ---- 4. the op's refusals, before any device call ---------------------------------------------------------------------------------
def test_ops_refuse_before_a_device_call():
    from multimodal_vae_comparison_amd import ops
    x = torch.rand(2, 3, 28, 28)
    cases = [
        (r"x is \(2, 3, 28\)", (x[:, :, 0], x), {}),
        ("y is .*int64", (x, x.long()), {}),
        ("x is list", ([1.0], x), {}),
        ("the same shape and device", (x, x[:1]), {}),
        ("win = 10", (x, x), {"win": 10}),
        ("win = 13", (x, x), {"win": 13}),
        ("win = 1 ", (x, x), {"win": 1}),
        ("planes of 28 x 10 for win = 11", (x[:, :, :, :10], x[:, :, :, :10]), {}),
        ("planes of 65 x 28", (torch.rand(1, 1, 65, 28), torch.rand(1, 1, 65, 28)), {}),
        ("5 channels", (torch.rand(1, 5, 28, 28), torch.rand(1, 5, 28, 28)), {}),
        ("0 images", (x[:0], x[:0]), {}),
        ("scales = 0", (x, x), {"scales": 0}),
        ("scales = 5", (x, x), {"scales": 5, "win": 3}),
        ("level 3 is 7 x 7, smaller than win = 11 .*scales <= 2", (x, x), {"scales": 3}),
        ("level 2 is 10 x 12, smaller than win = 11 .*scales <= 1", (x[:, :, :20, :24], x[:, :, :20, :24]), {"scales": 2}),
        ("level 1 is 27 x 28; pooling it into level 2 needs even sides", (x[:, :, :27], x[:, :, :27]), {"scales": 2, "win": 5}),
        ("level 2 is 14 x 7; pooling it into level 3", (x[:, :, :, :14], x[:, :, :, :14]), {"scales": 3, "win": 3}),
        ("sigma = 0", (x, x), {"sigma": 0.0}),
        ("data_range = 0", (x, x), {"data_range": 0}),
        ("k2 = -1", (x, x), {"k2": -1.0}),
        ("weights holds 3 values for scales = 2", (x, x), {"scales": 2, "weights": [0.2, 0.3, 0.5]}),
        ("weights holds 2 values", (x, x), {"scales": 2, "weights": [0.2, float("nan")]}),
        ("x is on cpu", (x, x), {}),
    ]
    for match, args, kwargs in cases:
        with pytest.raises(ValueError, match="image_quality: .*" + match):
            ops.image_quality(*args, **kwargs)


# ---- 5. the contract on CPU models ----------------------------------------------------------------------------------------------
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
        vae.reconstruction_quality()
    assert "unimodal" in str(e.value) and "TorchMMVAE.reconstruction_quality" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="reconstruction_quality needs eval mode"):
        model.reconstruction_quality([cdsprites_batch(4, 6, seed=3)])


def test_default_layouts():
    from multimodal_vae_comparison_amd.models.evaluation import EvaluationMixin as E
    t = torch.arange(2 * 3 * 32 * 32, dtype=torch.float32)
    assert E._image_planes((45, 27, 1)) is None and E._image_planes((4,)) is None
    assert torch.equal(E._image_planes((64, 64, 3))(torch.arange(2.0 * 12288).reshape(1, 2, 64, 64, 3)),
                       torch.arange(2.0 * 12288).reshape(2, 3, 64, 64))      # labelled by view, not permuted
    assert tuple(E._image_planes([28, 28, 1])(torch.zeros(1, 5, 28, 28, 1)).shape) == (5, 1, 28, 28)
    svhn = E._image_planes((32, 32, 3))
    nhwc = t.reshape(1, 2, 32, 32, 3)
    assert torch.equal(svhn(nhwc), t.reshape(2, 32, 32, 3).permute(0, 3, 1, 2))      # the decoder's output: permuted back
    assert torch.equal(svhn(t.reshape(2, 3, 32, 32)), t.reshape(2, 3, 32, 32))       # the batch's data: as it is


def test_argument_errors_come_before_the_first_forward(monkeypatch):
    from multimodal_vae_comparison_amd import synthetic
    model = _model()
    batch = synthetic.cdsprites_batch(4, 6, seed=3)
    calls = []
    monkeypatch.setattr(model, "forward", lambda *a, **kw: calls.append(1))
    who = "reconstruction_quality: .*"
    for match, args, kwargs in [
            (who + "`batches` is empty", ([],), {}),
            (who + "without data", ([dict(batch, mod_2=dict(batch["mod_2"], data=None))],), {}),
            (who + "`images` maps modalities", ([batch],), {"images": {}}),
            (who + "`images` maps modalities", ([batch],), {"images": {"mod_9": lambda t: t}}),
            (who + "`images` maps modalities", ([batch],), {"images": {"mod_1": 3}}),
            (who + r"must return float \(rows, C, H, W\)", ([batch],), {"images": {"mod_1": lambda t: t.reshape(len(t), -1)}}),
            ("image_quality: win = 4", ([batch],), {"win": 4}),
            ("image_quality: level 4 is 8 x 8, smaller than win = 11", ([batch],), {"scales": 4}),
            ("image_quality: planes of 3 x 27 for win = 11", ([batch],), {"images": {"mod_2": lambda t: t.reshape(-1, 1, 3, 27)}})]:
        with pytest.raises(ValueError, match=match):
            model.reconstruction_quality(*args, **kwargs)
    with pytest.raises(TypeError):
        model.reconstruction_quality([batch], window=7)
    text_only = _model(mods=[synthetic.CD_MODS[1], dict(synthetic.CD_MODS[1])])
    with pytest.raises(ValueError, match=who + "no modality of this model has a known image form"):
        text_only.reconstruction_quality([batch])
    assert not calls and model._eval_draws is False and model.eps_override is None


def test_a_failing_call_leaves_the_noise_setup_as_it_found_it():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    mine = model.eps_override = [torch.zeros(4, 8)]

    def broken(*a, **kw):
        assert model._eval_draws is True and not torch.is_grad_enabled()
        raise KeyError("forward fails inside the noise context")

    model.forward = broken
    with pytest.raises(KeyError):
        model.reconstruction_quality([cdsprites_batch(4, 6, seed=3)])
    assert model._eval_draws is False and torch.is_grad_enabled()
    assert model.eps_override is mine and len(mine) == 1
