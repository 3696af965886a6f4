"""csrc/image_quality.hip and TorchMMVAE.reconstruction_quality on the MI355X, held to the float64 numpy
restatement of tests/image_quality_reference.py (direct 2-D window sums; checked on the host against scipy's separable route)
within the rounding bars that module derives from its own denominators.  Nothing is held to the code under test."""
import numpy as np
import pytest
import torch

import image_quality_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
STATS = ("psnr", "ssim", "ms_ssim", "mse", "mae")


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def held(got, ref, what, ms=True):
    """every output within its bar of the restatement (printed first); `ms`: ms_ssim too, after the restatement alone has
    shown every clamped level value >= 0.05"""
    N, S = ref["levels"].shape
    assert set(got) == set(R.NAMES)
    for name in R.NAMES:
        assert got[name].dtype == torch.float64 and got[name].device.type == "cuda", name
        assert tuple(got[name].shape) == ((N, S) if name == "levels" else (N,)), (name, got[name].shape)
    g, bar = {k: v.cpu().numpy() for k, v in got.items()}, ref["bar"]
    for name in ("mse", "mae", "ssim", "levels"):
        e = np.abs(g[name] - ref[name]) / bar[name]
        print(f"{what}: {name} off by {e.max():.3g} bars (largest bar {bar[name].max():.3g})")
        assert e.max() <= 1.0, (what, name, e)
    fin = np.isfinite(ref["psnr"])
    assert np.array_equal(np.isposinf(g["psnr"]), ~fin), (what, g["psnr"], ref["psnr"])
    if fin.any():
        e = np.abs(g["psnr"][fin] - ref["psnr"][fin]) / bar["psnr"][fin]
        print(f"{what}: psnr off by {e.max():.3g} bars (largest bar {bar['psnr'][fin].max():.3g})")
        assert e.max() <= 1.0, (what, e)
    if ms:
        print(f"{what}: smallest clamped level value {ref['values'].min():.3g}")
        assert ref["values"].min() >= 0.05, "a level value near 0: the bar of ms_ssim says nothing there; choose other inputs"
        e = np.abs(g["ms_ssim"] - ref["ms_ssim"]) / bar["ms_ssim"]
        print(f"{what}: ms_ssim off by {e.max():.3g} bars (largest bar {bar['ms_ssim'].max():.3g})")
        assert e.max() <= 1.0, (what, e)


def same_bits(a, b):
    return all(torch.equal(a[name], b[name]) for name in R.NAMES)


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_against_the_restatement(ops, i):
    x, y, kw, ref = R.case(i)
    x, y = dev(x), dev(y)
    got = ops.image_quality(x, y, **kw)
    held(got, ref, R.IDS[i])
    again = ops.image_quality(x, y, **kw)
    assert same_bits(got, again), "two runs differ"


def test_a_row_does_not_depend_on_its_neighbours(ops):
    x, y, kw, _ = R.case(R.MANY)
    x, y = dev(x), dev(y)
    full = ops.image_quality(x, y, **kw)
    alone = ops.image_quality(x[:5].contiguous(), y[:5].contiguous(), **kw)
    assert all(torch.equal(alone[name], full[name][:5]) for name in R.NAMES)
    last = ops.image_quality(x[299:].contiguous(), y[299:].contiguous(), **kw)
    assert all(torch.equal(last[name], full[name][299:]) for name in R.NAMES)


def test_other_dtypes_and_strides_are_read_as_fp32(ops):
    x, y, kw, _ = R.case(4)
    x, y = dev(x), dev(y)
    want = ops.image_quality(x, y, **kw)
    assert same_bits(want, ops.image_quality(x.double(), y.double(), **kw))
    xt = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not xt.is_contiguous() and same_bits(want, ops.image_quality(xt, y, **kw))


@pytest.mark.parametrize("i", [4, 5, 1])
def test_identical_images(ops, i):
    x, _, kw, _ = R.case(i)
    ref = R.image_quality(x, x, **kw)
    got = ops.image_quality(dev(x), dev(x), **kw)
    assert bool((got["mse"] == 0.0).all()) and bool((got["mae"] == 0.0).all()) and bool(torch.isposinf(got["psnr"]).all())
    assert np.all(np.abs(got["ssim"].cpu().numpy() - 1.0) <= ref["bar"]["ssim"])
    held(got, ref, f"{R.IDS[i]} against itself")


def test_a_negative_has_ms_ssim_zero(ops):
    x, y = R.anti_correlated()
    for kw in (dict(win=11, scales=2), dict(win=11), dict(win=7, scales=2, sigma=None)):
        ref = R.image_quality(x, y, **kw)
        assert np.all(ref["ms_ssim"] == 0.0) and np.all(ref["levels"][:, 0] < 0.0 if "scales" in kw else ref["ssim"] < 0.0)
        got = ops.image_quality(dev(x), dev(y), **kw)
        assert bool((got["ms_ssim"] == 0.0).all()), got["ms_ssim"]
        held(got, ref, f"negative {kw}", ms=False)


def test_the_limits_raise(ops):
    x = torch.rand(2, 3, 28, 28, device=DEV)
    nan = x.clone()
    nan[1, 2, 27, 27] = float("nan")
    inf = x.clone()
    inf[0, 0, 0, 0] = float("inf")
    for match, args, kwargs in [
            ("win = 10", (x, x), {"win": 10}),
            ("planes of 28 x 10 for win = 11", (x[..., :10], x[..., :10]), {}),
            ("level 1 is 27 x 28; pooling it into level 2 needs even sides", (x[:, :, :27], x[:, :, :27]), {"scales": 2, "win": 5}),
            ("level 3 is 7 x 7, smaller than win = 11", (x, x), {"scales": 3}),
            ("scales = 5", (x, x), {"scales": 5, "win": 3}),
            ("the same shape and device", (x, x[:, :2]), {}),
            ("the same shape and device", (x, x.cpu()), {}),
            ("y holds values that are not finite", (x, nan), {}),
            ("x holds values that are not finite", (inf, x), {})]:
        with pytest.raises(ValueError, match="image_quality: .*" + match):
            ops.image_quality(*args, **kwargs)


def test_c_entry_point_refuses_and_writes_nothing(ops):
    import ctypes
    from multimodal_vae_comparison_amd import hipops as H
    x = torch.rand(2, 4, 64, 64, device=DEV)
    out = torch.full((64,), -1.0, dtype=torch.float64, device=DEV)
    g, w = (ctypes.c_double * 11)(*([1.0 / 11] * 11)), (ctypes.c_double * 4)(*([0.25] * 4))
    L, s, p = H.lib(), H.stream(), H.ptr
    # (N, C, H, W, win, scales)
    for N, C, Hh, W, win, S in ((0, 1, 64, 64, 11, 1), (2, 0, 64, 64, 11, 1), (2, 5, 32, 32, 11, 1), (2, 1, 65, 64, 11, 1),
                                (2, 1, 64, 65, 11, 1), (2, 1, 64, 10, 11, 1), (2, 1, 64, 64, 10, 1), (2, 1, 64, 64, 13, 1),
                                (2, 1, 64, 64, 1, 1), (2, 1, 64, 64, 11, 0), (2, 1, 64, 64, 11, 4), (2, 1, 64, 64, 3, 5),
                                (2, 1, 20, 20, 11, 2), (2, 1, 27, 28, 5, 2), (2, 1, 28, 28, 11, 3)):
        rc = L.mmvae_image_quality(p(x), p(x), p(out), N, C, Hh, W, win, g, 1.0, 1e-4, 9e-4, 1.0, S, w, s)
        assert rc == H.ERR_UNSUPPORTED, (N, C, Hh, W, win, S, rc)
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    assert L.mmvae_image_quality(p(x), p(x), p(out), 2, 4, 64, 64, 11, g, 1.0, 1e-4, 9e-4, 1.0, 3, w, s) == 0
    torch.cuda.synchronize()
    assert bool((out[:16].reshape(2, 8)[:, :2] == 0.0).all()) and bool((out[16:] == -1.0).all())


# ---- 2. the metric end to end ---------------------------------------------------------------------------------------------------------
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


def _optimizer_state(tr):
    """the optimiser's step count and moment buffers"""
    state = tr.optimizer.state_dict()["state"]
    return [(k, n, v.clone() if torch.is_tensor(v) else v) for k, st in state.items() for n, v in st.items()]


def _same_optimizer_state(a, b):
    assert len(a) == len(b)
    for (ka, na, va), (kb, nb, vb) in zip(a, b):
        assert (ka, na) == (kb, nb) and (torch.equal(va, vb) if torch.is_tensor(va) else va == vb), "the optimiser's state changed"


def _decoded(model, m, like, seed):
    """`real` images of modality m that lie where the model generates: decodings of seeded prior latents, shaped as `like`
    (an NCHW batch; a decoder that returns channels last is permuted back)"""
    g = torch.Generator().manual_seed(seed)
    loc, scale = model.pz_params
    z = (loc + scale * torch.randn(len(like), model.n_latents, generator=g).to(DEV)).unsqueeze(0).contiguous()
    with torch.no_grad():
        out = model.vaes[m].dec({"latents": z, "masks": None})[0].detach()
    if tuple(out.shape[-3:]) == (32, 32, 3):
        out = out.reshape(-1, 32, 32, 3).permute(0, 3, 1, 2)
    return out.reshape(like.shape).contiguous().clone()


def _forwards(model, batches, eps, mods):
    """forward() by hand through eps_override, in the metric's order: per batch the full batch, then only g given for every
    modality g that some modality of `mods` is generated from -> per batch (full, {g: only g given})"""
    outs = []
    with torch.no_grad():
        model.eps_override = [e.clone() for e in eps]
        for b in batches:
            full = model.forward(b)
            outs.append((full, {g: model.forward(model._given_only(b, [g])) for g in model.vaes if any(m != g for m in mods)}))
        model.eps_override = None
    return outs


def _np(t):
    return t.detach().float().cpu().numpy()


def _check_set(got_means, got_per, real, gen, kw, what):
    ref = R.image_quality(real, gen, **kw)
    held(got_per, ref, what, ms=kw.get("scales", 1) > 1)
    assert set(got_means) == set(STATS) and all(isinstance(v, float) for v in got_means.values())
    for name in STATS:
        assert got_means[name] == float(got_per[name].mean()), (what, name)
    return ref


def test_reconstruction_quality_cdsprites(ops):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch, config_from_mods
    B, D, kw = 5, 8, dict(scales=3)
    torch.manual_seed(31)
    cfg, dims = config_from_mods("mopoe", CD_MODS, D, batch_size=B)
    tr = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0")
    model = tr.model
    model.eval()
    batches = [cdsprites_batch(B, 6, seed=s, device=DEV) for s in (3, 4)]
    batches = [dict(b, mod_1=dict(b["mod_1"], data=_decoded(model, "mod_1", b["mod_1"]["data"], 40 + i)))
               for i, b in enumerate(batches)]
    g = torch.Generator().manual_seed(33)
    eps = [torch.randn(B, D, generator=g) for _ in range(32)]
    tr.configure_optimizers()
    model.objective(batches[0])["loss"].backward()      # a gradient to watch
    torch.cuda.synchronize()
    before, opt_before = _state(model), _optimizer_state(tr)

    out = tr.reconstruction_quality(batches, eps=[e.clone() for e in eps], **kw)
    torch.cuda.synchronize()
    _same_state(before, _state(model))
    _same_optimizer_state(opt_before, _optimizer_state(tr))
    assert model.eps_override is None and model._eval_draws is False and torch.is_grad_enabled()
    assert set(out) == {"mod_1"}
    r = out["mod_1"]
    assert set(r) == {"recon", "cross", "n", "shape", "per_sample"} and (r["n"], r["shape"]) == (2 * B, (3, 64, 64))
    assert set(r["cross"]) == {"mod_2"} and set(r["per_sample"]) == {"recon", "cross"} and set(r["per_sample"]["cross"]) == {"mod_2"}

    outs = _forwards(model, batches, eps, ["mod_1"])
    real = np.concatenate([_np(b["mod_1"]["data"]).reshape(-1, 3, 64, 64) for b in batches])
    recon = np.concatenate([_np(full.mods["mod_1"].decoder_dist.loc).reshape(-1, 3, 64, 64)[:B] for full, _ in outs])
    cross = np.concatenate([_np(only["mod_2"].mods["mod_1"].decoder_dist.loc).reshape(-1, 3, 64, 64)[:B] for _, only in outs])
    a = _check_set(r["recon"], r["per_sample"]["recon"], real, recon, kw, "cdsprites recon")
    b = _check_set(r["cross"]["mod_2"], r["per_sample"]["cross"]["mod_2"], real, cross, kw, "cdsprites from mod_2")
    assert not np.array_equal(a["ssim"], b["ssim"]), "the two sets give the same numbers: choose another seed"
    logged = {key: float(v) for key, v in tr.logged.items() if key.startswith(("test_psnr", "test_ssim", "test_ms_ssim"))}
    assert logged == {f"test_{name}_mod_1_{tag}": d[name] for tag, d in (("recon", r["recon"]), ("from_mod_2", r["cross"]["mod_2"]))
                      for name in ("psnr", "ssim", "ms_ssim")}

    model.train()
    with pytest.raises(RuntimeError, match="reconstruction_quality needs eval mode"):
        tr.reconstruction_quality(batches)
    model.eval()


def test_reconstruction_quality_mnist_svhn(ops):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import MS_MODS, config_from_mods, mnist_svhn_batch
    B, D, kw = 5, 8, dict(win=7, scales=2)
    torch.manual_seed(35)
    cfg, dims = config_from_mods("moe", MS_MODS, D, batch_size=B)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cuda:0").model
    model.eval()
    batches = [mnist_svhn_batch(B, seed=s, device=DEV) for s in (5, 6)]
    batches = [{m: dict(v, data=_decoded(model, m, v["data"], 50 + 2 * i + j)) for j, (m, v) in enumerate(b.items())}
               for i, b in enumerate(batches)]
    g = torch.Generator().manual_seed(37)
    eps = [torch.randn(B, D, generator=g) for _ in range(32)]
    before = _state(model)
    out = model.reconstruction_quality(batches, eps=[e.clone() for e in eps], **kw)
    torch.cuda.synchronize()
    _same_state(before, _state(model))
    assert set(out) == {"mod_1", "mod_2"}
    assert (out["mod_1"]["shape"], out["mod_2"]["shape"]) == ((1, 28, 28), (3, 32, 32)) and out["mod_1"]["n"] == 2 * B
    outs = _forwards(model, batches, eps, ["mod_1", "mod_2"])

    def mnist(t):
        return _np(t).reshape(-1, 1, 28, 28)

    def svhn(t):      # the decoder returns (.., 32, 32, 3); the batch holds (B, 3, 32, 32)
        t = _np(t)
        return t.reshape(-1, 32, 32, 3).transpose(0, 3, 1, 2) if t.shape[-3:] == (32, 32, 3) else t.reshape(-1, 3, 32, 32)

    for m, other, planes in (("mod_1", "mod_2", mnist), ("mod_2", "mod_1", svhn)):
        r = out[m]
        real = np.concatenate([planes(b[m]["data"]) for b in batches])
        recon = np.concatenate([planes(full.mods[m].decoder_dist.loc)[:B] for full, _ in outs])
        cross = np.concatenate([planes(only[other].mods[m].decoder_dist.loc)[:B] for _, only in outs])
        assert set(r["cross"]) == {other}
        _check_set(r["recon"], r["per_sample"]["recon"], real, recon, kw, f"{m} recon")
        _check_set(r["cross"][other], r["per_sample"]["cross"][other], real, cross, kw, f"{m} from {other}")
    # SVHN: the planes are the permuted ones -- read as (3, 32, 32) without the permutation the decoder's output scores
    # differently, far beyond the bars
    assert tuple(outs[0][0].mods["mod_2"].decoder_dist.loc.shape[-3:]) == (32, 32, 3)
    real = np.concatenate([svhn(b["mod_2"]["data"]) for b in batches])
    wrong = np.concatenate([_np(full.mods["mod_2"].decoder_dist.loc).reshape(-1, 3, 32, 32)[:B] for full, _ in outs])
    ref = R.image_quality(real, wrong, **kw)
    got = out["mod_2"]["per_sample"]["recon"]["ssim"].cpu().numpy()
    gap = np.abs(got - ref["ssim"])
    print(f"SVHN read without the permutation: ssim differs by {gap.min():.3g} .. {gap.max():.3g} (bar {ref['bar']['ssim'].max():.3g})")
    assert gap.min() > 1e3 * ref["bar"]["ssim"].max()
