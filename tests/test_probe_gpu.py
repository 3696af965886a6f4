"""GPU checks of latent classification (csrc/probe.hip, ops.probe_*, TorchMMVAE.latents_for / classify_latents).

Yardstick, restated here: torch.nn.Linear + torch.nn.CrossEntropyLoss + torch.optim.Adam(lr) on the CPU in float64 -- the
library objects the reference's classifier loop calls (eval/eval_mnistsvhn.py:24-67) -- with the same init, the same rows
in the same order.  Bars, relative to the tensor's largest magnitude (`check` of test_loglik_gpu.py): parameters, both Adam
moments and the per-step loss curve 1e-5; per-row test cross-entropy 1e-5; predictions equal except on rows whose float64
top-two logit gap is <= 1e-5 of the largest |logit|, at most 2 rows per case.  The same restatement in float32 on the CPU
ends within 3.7e-7 .. 1.7e-6 (W) and 4.8e-8 .. 2.3e-6 (b) of float64 on these shapes: every parity test first asserts that
figure <= 2.5e-6, so that an ill-conditioned input cannot excuse the kernel."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64

# (N, D, C, batch, epochs); the last has a short final minibatch of 18 rows
SHAPES = [(4096, 32, 10, 128, 5), (4000, 16, 10, 128, 30), (1000, 256, 32, 100, 10), (4096, 20, 10, 256, 20),
          (530, 32, 3, 64, 8)]
LR = 1e-3


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def check(a, b, tol, what):
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    e = rel_err(a, b)
    print(f"{what}: rel err {e:.3e} (bar {tol})")
    assert math.isfinite(e) and e <= tol, f"{what}: rel err {e:.3e} > {tol}"


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


@pytest.fixture(scope="module")
def H(hip_lib):
    from multimodal_vae_comparison_amd import hipops
    return hipops


def _data(N, D, C, seed):
    """latents = class centres x 0.7 + unit noise"""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(C, D, generator=g)
    y = torch.randint(0, C, (N,), generator=g)
    z = 0.7 * centres[y] + torch.randn(N, D, generator=g)
    return z, y, centres


def _init(D, C, seed):
    g = torch.Generator().manual_seed(seed)
    bound = 1.0 / math.sqrt(D)
    return (torch.rand(C, D, generator=g) * 2 - 1) * bound, (torch.rand(C, generator=g) * 2 - 1) * bound


def _ref_train(z, y, W0, b0, batch, epochs, lr, order=None, dtype=F64):
    """the restatement -> dict of W, b, mW, mb, vW, vb and the per-step loss curve"""
    C, D = W0.shape
    lin = torch.nn.Linear(D, C).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(W0.to(dtype))
        lin.bias.copy_(b0.to(dtype))
    opt = torch.optim.Adam(lin.parameters(), lr=lr)
    ce = torch.nn.CrossEntropyLoss()
    z = z.to(dtype)
    N, curve = z.shape[0], []
    for e in range(epochs):
        idx = torch.arange(N) if order is None else order[e].long()
        for i in range(0, N, batch):
            rows = idx[i:i + batch]
            opt.zero_grad()
            loss = ce(lin(z[rows]), y[rows])
            loss.backward()
            opt.step()
            curve.append(float(loss.detach()))
    sw, sb = opt.state[lin.weight], opt.state[lin.bias]
    return {"W": lin.weight.detach(), "b": lin.bias.detach(), "mW": sw["exp_avg"], "mb": sb["exp_avg"],
            "vW": sw["exp_avg_sq"], "vb": sb["exp_avg_sq"], "loss": torch.tensor(curve, dtype=F64), "lin": lin}


def _assert_fp32_room(z, y, W0, b0, batch, epochs, ref, order=None):
    """the fp32-CPU-vs-fp64 figure of this input, asserted <= 2.5e-6 before the kernel is looked at"""
    r32 = _ref_train(z, y, W0, b0, batch, epochs, LR, order=order, dtype=torch.float32)
    eW, eb = rel_err(r32["W"], ref["W"]), rel_err(r32["b"], ref["b"])
    print(f"fp32 CPU vs fp64: W {eW:.3e}, b {eb:.3e} (bar 2.5e-6)")
    assert eW <= 2.5e-6 and eb <= 2.5e-6, (eW, eb)
    return r32


def _device_train(ops, z, y, W0, b0, batch, epochs, order=None, splits=None):
    """one probe on the device -> (state, loss curve (steps,)); `splits`: step counts of consecutive launches"""
    N, D = z.shape
    C = W0.shape[0]
    st = ops.probe_state(1, D, C, DEV, init=[(W0, b0)])
    zg, yg = z.reshape(1, N, D).to(DEV).contiguous(), y.reshape(1, N).to(device=DEV, dtype=torch.int32)
    og = None if order is None else order.to(device=DEV, dtype=torch.int32).contiguous()
    steps = epochs * ((N + batch - 1) // batch)
    curve, t = [], 0
    for n in (splits or [steps]):
        curve.append(ops.probe_train(st, zg, yg, [(0, 0, C)], batch, t, n, lr=LR, order=og))
        t += n
    assert t == steps
    torch.cuda.synchronize()
    return st, torch.cat(curve, 1)[0]


def _check_state(ops, st, curve, ref, tag):
    C = ref["W"].shape[0]
    for k, (nw, nb) in enumerate((("W", "b"), ("mW", "mb"), ("vW", "vb"))):
        check(st[0, k, :C, :-1], ref[nw], 1e-5, f"{tag} {nw}")
        check(st[0, k, :C, -1], ref[nb], 1e-5, f"{tag} {nb}")
    check(curve, ref["loss"], 1e-5, f"{tag} loss curve")
    W, b = ops.probe_weights(st, 0, C)
    assert torch.equal(W, st[0, 0, :C, :-1]) and torch.equal(b, st[0, 0, :C, -1])


# ---------------------------------------------------------------------------------------------
# 1. training parity, one probe
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,C,batch,epochs", SHAPES)
def test_training_parity(ops, N, D, C, batch, epochs):
    z, y, _ = _data(N, D, C, seed=N + D)
    W0, b0 = _init(D, C, seed=C)
    ref = _ref_train(z, y, W0, b0, batch, epochs, LR)
    _assert_fp32_room(z, y, W0, b0, batch, epochs, ref)
    st, curve = _device_train(ops, z, y, W0, b0, batch, epochs)
    _check_state(ops, st, curve, ref, f"({N},{D},{C},{batch},{epochs})")


# ---------------------------------------------------------------------------------------------
# 2. many probes in one launch
# ---------------------------------------------------------------------------------------------
def test_many_probes_equal_single_probe_launches_bit_for_bit(ops):
    N, D, batch, epochs, Cs = 1000, 32, 128, 3, (3, 10, 32)
    g = torch.Generator().manual_seed(11)
    z = torch.randn(2, N, D, generator=g)
    labels = torch.stack([torch.randint(0, C, (N,), generator=g) for C in Cs]).int()
    probes = [(s, a, Cs[a]) for s in range(2) for a in range(3)]
    zg, lg = z.to(DEV), labels.to(DEV)
    st0 = ops.probe_state(6, D, 32, DEV, seed=3)
    steps = epochs * ((N + batch - 1) // batch)
    many = st0.clone()
    loss = ops.probe_train(many, zg, lg, probes, batch, 0, steps, lr=LR)
    for p, pr in enumerate(probes):
        one = st0[p:p + 1].clone()
        l1 = ops.probe_train(one, zg, lg, [pr], batch, 0, steps, lr=LR)
        torch.cuda.synchronize()
        assert torch.equal(one[0], many[p]), f"probe {p} {pr}: state differs from its single-probe launch"
        assert torch.equal(l1[0], loss[p]), f"probe {p} {pr}: loss curve differs"
        C = pr[2]
        assert torch.equal(many[p, :, C:], st0[p, :, C:]), f"probe {p}: classes >= {C} were touched"
        assert not torch.equal(many[p, 0, :C], st0[p, 0, :C])
    # and the largest one against float64
    p = 5
    W0, b0 = ops.probe_weights(st0, p, 32)
    ref = _ref_train(z[1], labels[2].long(), W0.cpu(), b0.cpu(), batch, epochs, LR)
    check(many[p, 0, :, :-1], ref["W"], 1e-5, "P = 6, probe 5 W")
    check(loss[p], ref["loss"], 1e-5, "P = 6, probe 5 loss curve")


# ---------------------------------------------------------------------------------------------
# 3. resumption
# ---------------------------------------------------------------------------------------------
def test_split_launches_are_bit_identical(ops):
    N, D, C, batch, epochs = 530, 32, 3, 64, 5
    z, y, _ = _data(N, D, C, seed=5)
    W0, b0 = _init(D, C, seed=6)
    spe = (N + batch - 1) // batch
    whole, c0 = _device_train(ops, z, y, W0, b0, batch, epochs)
    again, c1 = _device_train(ops, z, y, W0, b0, batch, epochs)
    assert torch.equal(whole, again) and torch.equal(c0, c1), "two identical runs differ"
    per_epoch, c2 = _device_train(ops, z, y, W0, b0, batch, epochs, splits=[spe] * epochs)
    assert torch.equal(whole, per_epoch) and torch.equal(c0, c2), "one launch per epoch differs from one launch"
    mid, c3 = _device_train(ops, z, y, W0, b0, batch, epochs, splits=[4, 13, 1, epochs * spe - 18])
    assert torch.equal(whole, mid) and torch.equal(c0, c3), "launches split mid-epoch differ from one launch"
    # rows tiled inside a step (batch > the tile's rows at D = 256) resume the same way
    N, D, C, batch, epochs = 300, 256, 5, 100, 2
    z, y, _ = _data(N, D, C, seed=8)
    W0, b0 = _init(D, C, seed=9)
    a, ca = _device_train(ops, z, y, W0, b0, batch, epochs)
    b, cb = _device_train(ops, z, y, W0, b0, batch, epochs, splits=[1, 2, 3])
    assert torch.equal(a, b) and torch.equal(ca, cb)


# ---------------------------------------------------------------------------------------------
# 4. order
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,C,batch,epochs", [SHAPES[0], SHAPES[4]])
def test_order(ops, N, D, C, batch, epochs):
    z, y, _ = _data(N, D, C, seed=N + 1)
    W0, b0 = _init(D, C, seed=C + 1)
    g = torch.Generator().manual_seed(N)
    order = torch.stack([torch.randperm(N, generator=g) for _ in range(epochs)])
    ref = _ref_train(z, y, W0, b0, batch, epochs, LR, order=order)
    _assert_fp32_room(z, y, W0, b0, batch, epochs, ref, order=order)
    st, curve = _device_train(ops, z, y, W0, b0, batch, epochs, order=order)
    _check_state(ops, st, curve, ref, f"order ({N},{D},{C},{batch},{epochs})")
    ident = torch.arange(N).expand(epochs, N).contiguous()
    si, ci = _device_train(ops, z, y, W0, b0, batch, epochs, order=ident)
    sn, cn = _device_train(ops, z, y, W0, b0, batch, epochs)
    assert torch.equal(si, sn) and torch.equal(ci, cn), "NULL order differs from the identity permutation"
    assert not torch.equal(st, sn)


# ---------------------------------------------------------------------------------------------
# 5. the evaluation kernel
# ---------------------------------------------------------------------------------------------
def _check_eval(pred, nll, W, b, z, y, tag):
    """pred / nll of the device against float64 with the SAME parameters -> number of excused rows"""
    logits = z.double() @ W.double().t() + b.double()
    ref_nll = torch.nn.functional.cross_entropy(logits, y, reduction="none")
    check(nll, ref_nll, 1e-5, f"{tag} nll")
    ref_pred = logits.argmax(1)
    bad = (pred.cpu().long() != ref_pred).nonzero().flatten()
    top2 = logits.topk(2, 1).values
    gap = (top2[:, 0] - top2[:, 1])[bad]
    lim = 1e-5 * float(logits.abs().max())
    print(f"{tag}: {bad.numel()} rows differ from the float64 argmax (gaps {gap.tolist()}, limit {lim:.3e})")
    assert bad.numel() <= 2 and bool((gap <= lim).all()), (bad.tolist(), gap.tolist(), lim)
    p32 = (z @ W.float().t() + b.float()).argmax(1)
    n32 = int((p32 != ref_pred).sum())
    print(f"{tag}: fp32 CPU disagreements with float64: {n32}")
    assert n32 == 0, f"{tag}: the fp32 CPU restatement itself flips {n32} predictions: the allowance below would be hollow"
    return bad.numel()


@pytest.mark.parametrize("N,D,C,batch,epochs", SHAPES)
def test_eval_kernel(ops, N, D, C, batch, epochs):
    z, y, centres = _data(N, D, C, seed=N + D)
    W0, b0 = _init(D, C, seed=C)
    st, _ = _device_train(ops, z, y, W0, b0, batch, epochs)
    g = torch.Generator().manual_seed(99)
    Nt = 2049
    yt = torch.randint(0, C, (Nt,), generator=g)
    zt = 0.7 * centres[yt] + torch.randn(Nt, D, generator=g)
    pred, nll = ops.probe_eval(st, zt.reshape(1, Nt, D).to(DEV), yt.reshape(1, Nt).int().to(DEV), [(0, 0, C)])
    torch.cuda.synchronize()
    assert pred.shape == (1, Nt) and pred.dtype == torch.int32 and nll.shape == (1, Nt)
    W, b = ops.probe_weights(st, 0, C)
    _check_eval(pred[0], nll[0], W.cpu(), b.cpu(), zt, yt, f"eval ({N},{D},{C})")
    # without labels: the same predictions
    pred2, _ = ops.probe_eval(st, zt.reshape(1, Nt, D).to(DEV), None, [(0, 0, C)])
    assert torch.equal(pred, pred2)


def test_eval_exact_tie_picks_the_lower_index(ops):
    D, C, N = 20, 6, 700
    W0, b0 = _init(D, C, seed=1)
    W0[4], b0[4] = W0[1], b0[1]
    st = ops.probe_state(1, D, C, DEV, init=[(W0, b0)])
    z = torch.randn(1, N, D, generator=torch.Generator().manual_seed(2))
    pred, _ = ops.probe_eval(st, z.to(DEV), None, [(0, 0, C)])
    pred = pred[0].cpu()
    ref = (z[0].double() @ W0.double().t() + b0.double()).argmax(1)
    n_tie = int(((ref == 1) | (ref == 4)).sum())
    assert n_tie > 20, "the case must hold rows whose maximum is the duplicated class"
    assert int((pred == 4).sum()) == 0 and int((pred == 1).sum()) == n_tie


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["D257", "C1", "C33", "batch0", "s_range", "a_range"])
def test_refusals_write_nothing(ops, H, hip_lib, what):
    import ctypes
    N, S, A = 64, 2, 2
    D = 257 if what == "D257" else 16
    Cmax = 32
    probe = {"C1": (0, 0, 1), "C33": (0, 0, 33), "s_range": (S, 0, 4), "a_range": (0, A, 4)}.get(what, (0, 0, 4))
    batch = 0 if what == "batch0" else 16
    state = torch.full((1, 3, Cmax, D + 1), 7.0, device=DEV)
    z = torch.zeros(S, N, D, device=DEV)
    labels = torch.zeros(A, N, dtype=torch.int32, device=DEV)
    loss = torch.full((1, 4), 7.0, device=DEV)
    pred = torch.full((1, N), 7, dtype=torch.int32, device=DEV)
    nll = torch.full((1, N), 7.0, device=DEV)
    table = (ctypes.c_int * 3)(*probe)
    rc = hip_lib.mmvae_probe_train(H.ptr(state), H.ptr(z), H.ptr(labels), None, 0, table, H.ptr(loss), 1, S, A, N, D, Cmax,
                                   batch, 0, 4, 1e-3, H.stream())
    assert rc == 2, rc
    if what != "batch0":      # (the evaluation has no batch)
        rc = hip_lib.mmvae_probe_eval(H.ptr(state), H.ptr(z), H.ptr(labels), table, H.ptr(pred), H.ptr(nll), 1, S, A, N, D,
                                      Cmax, H.stream())
        assert rc == 2, rc
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((loss == 7.0).all()) and bool((pred == 7).all()) and bool((nll == 7.0).all())
    # the Python layer names the reason before any launch
    if what in ("C1", "C33"):
        with pytest.raises(ValueError, match="classes"):
            ops.probe_train(state, z, labels, [probe], batch, 0, 4)
    if what == "D257":
        with pytest.raises(ValueError, match="257"):
            ops.probe_train(state, z, labels, [probe], batch, 0, 4)
    if what in ("s_range", "a_range"):
        with pytest.raises(ValueError, match="outside|label row"):
            ops.probe_train(state, z, labels, [probe], batch, 0, 4)


def test_label_outside_the_class_count_raises_before_the_launch(ops):
    N, D = 64, 16
    state = torch.full((1, 3, 4, D + 1), 7.0, device=DEV)
    z = torch.zeros(1, N, D, device=DEV)
    labels = torch.zeros(1, N, dtype=torch.int32, device=DEV)
    labels[0, 3] = 4
    with pytest.raises(ValueError, match="labels"):
        ops.probe_train(state, z, labels, [(0, 0, 4)], 16, 0, 4)
    torch.cuda.synchronize()
    assert bool((state == 7.0).all())


# ---------------------------------------------------------------------------------------------
# 7. latents_for
# ---------------------------------------------------------------------------------------------
def _to_dev(batch):
    return {k: {kk: (vv.to(DEV) if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in batch.items()}


def _model(mixing, D=16, B=5):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import (CD_MODS, MS_MODS, cdsprites_batch, config_from_mods,
                                                         mnist_svhn_batch)
    torch.manual_seed(0)
    if mixing == "dmvae":
        mods, batch = [dict(m, private=4) for m in MS_MODS], mnist_svhn_batch(B, seed=2)
    else:
        mods, batch = CD_MODS, cdsprites_batch(B, 8, seed=2)
    cfg, dims = config_from_mods(mixing, mods, D, batch_size=B)
    tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
    tr.model.eval()
    return tr, _to_dev(batch)


@pytest.mark.parametrize("mixing", ["poe", "moe", "mopoe", "dmvae"])
def test_latents_for_equals_forward_bit_for_bit(hip_lib, mixing):
    tr, batch = _model(mixing)
    model = tr.model
    names = list(model.vaes.keys())
    B, D = 5, model.n_latents
    for given in [[n] for n in names] + [names]:
        x = model._given_only(batch, given)
        shapes = []
        orig = model._draw

        def rec(b, d, dev):
            shapes.append((b, d))
            return orig(b, d, dev)
        model._draw = rec      # the draws forward() takes for this input, in order
        try:
            with torch.no_grad():
                model.forward(x)
        finally:
            del model._draw
        g = torch.Generator().manual_seed(len(given) + 7)
        eps = [torch.randn(1, b, d, generator=g) for b, d in shapes]
        model.eps_override = [e.clone() for e in eps]
        with torch.no_grad():
            out = model.forward(x)
        assert model.eps_override == []
        for of in names:
            want = out.mods[of].latent_samples["latents"]
            model.eps_override = [e.clone() for e in eps]
            got = model.latents_for(batch, given, of=of)
            model.eps_override = None
            assert got.shape == (B, D) and want.numel() == B * D
            assert torch.equal(got, want.reshape(B, D)), f"{mixing} given={given} of={of}"
        model.eps_override = [e.clone() for e in eps]
        assert torch.equal(model.latents_for(batch, given), out.mods[given[0]].latent_samples["latents"].reshape(B, D))
        model.eps_override = None
        # the generator path: the training noise state stays, the evaluation one moves
        before, ev = model._rng_state.clone(), model._eval_rng_state.clone()
        a = model.latents_for(batch, given)
        b = model.latents_for(batch, given)
        torch.cuda.synchronize()
        assert torch.equal(model._rng_state, before), "the training noise state moved"
        assert not torch.equal(model._eval_rng_state, ev)
        assert not torch.equal(a, b), "a second call draws fresh noise"
        assert not a.requires_grad and bool(torch.isfinite(a).all())


def _forward_recording_draws(model, x, K=1):
    """forward(x, K) -> (its output, the (B, d) shapes it asked `_draw` for, in order)"""
    shapes, orig = [], model._draw

    def rec(b, d, dev):
        shapes.append((b, d))
        return orig(b, d, dev)
    model._draw = rec
    try:
        with torch.no_grad():
            out = model.forward(x, K=K)
    finally:
        del model._draw
    return out, shapes


# the reference's draw order (models/mmvae_models.py: poe :189-208, mopoe :351-370, moe :80-117, dmvae :467-503) for the two
# modalities of `_model`, keyed by which of them carry data.  S = a latent-wide draw (B, D), P = a private one (B, 4).
# dmvae: z_joint, then per modality z_shared, z_private and a fresh shared draw of every OTHER PRESENT modality.
_S, _P = (5, 16), (5, 4)
REFERENCE_DRAWS = {
    "poe": {"0": [_S], "1": [_S], "01": [_S]},
    "mopoe": {"0": [_S, _S], "1": [_S, _S], "01": [_S, _S]},
    "moe": {"0": [_S], "1": [_S], "01": [_S, _S]},
    "dmvae": {"0": [_S, _S, _P, _S, _P, _S], "1": [_S, _S, _P, _S, _S, _P], "01": [_S, _S, _P, _S, _S, _P, _S]},
}


@pytest.mark.parametrize("mixing", ["poe", "moe", "mopoe", "dmvae"])
def test_forward_draw_order_is_the_references(hip_lib, mixing):
    tr, batch = _model(mixing)
    model = tr.model
    names = list(model.vaes.keys())
    assert len(names) == 2 and model.n_latents == 16
    for key, want in REFERENCE_DRAWS[mixing].items():
        x = model._given_only(batch, [names[int(c)] for c in key])
        _, got = _forward_recording_draws(model, x)
        print(f"{mixing} given {key}: {got}")
        assert got == want, f"{mixing} given {key}: {got} != {want}"
        if mixing != "dmvae":      # K = 2: every entry twice in a row
            _, got = _forward_recording_draws(model, x, K=2)
            print(f"{mixing} given {key} K = 2: {got}")
            assert got == [s for s in want for _ in range(2)], f"{mixing} given {key} K = 2: {got}"


@pytest.mark.parametrize("mixing", ["poe", "moe", "mopoe", "dmvae"])
def test_forward_k2_slices_equal_k1_forward_on_the_same_draws(hip_lib, mixing):
    tr, batch = _model(mixing)
    model = tr.model
    names = list(model.vaes.keys())
    B, D = 5, model.n_latents
    if mixing == "dmvae":
        with pytest.raises(NotImplementedError):
            model.forward(batch, K=2)
        return
    for given in [[n] for n in names] + [names]:
        x = model._given_only(batch, given)
        _, shapes = _forward_recording_draws(model, x, K=2)
        g = torch.Generator().manual_seed(len(given) + 11)
        eps = [torch.randn(1, b, d, generator=g) for b, d in shapes]      # draws 2 i, 2 i + 1: k = 0, 1 of the i-th block
        model.eps_override = [e.clone() for e in eps]
        with torch.no_grad():
            out2 = model.forward(x, K=2)
        assert model.eps_override == []
        for k in range(2):
            model.eps_override = [e.clone() for e in eps[k::2]]
            with torch.no_grad():
                out1 = model.forward(x)
            assert model.eps_override == []
            for of in names:
                z2 = out2.mods[of].latent_samples["latents"]
                z1 = out1.mods[of].latent_samples["latents"]
                assert z2.shape == (2, B, D) and z1.shape == (1, B, D), (z2.shape, z1.shape)
                assert torch.equal(z2[k], z1[0]), f"{mixing} given={given} of={of} k={k}"
        model.eps_override = None


# ---------------------------------------------------------------------------------------------
# 8. no footprint on training
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("captured", [True, False])
def test_classification_between_steps_leaves_training_bit_identical(hip_lib, captured):
    """three training steps of the cfg2-shaped MoPoE with and without a classify_latents between the steps (the pattern of
    test_loglik_gpu.test_estimate_between_steps_leaves_training_bit_identical)"""
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import workload
    res = []
    seed0 = DropoutState._next_seed[0]
    try:
        for evaluate in (False, True):
            torch.manual_seed(0)
            DropoutState._next_seed[0] = 0x1234567
            _, cfg, dims, data, _ = workload("cfg2", 32, device=DEV, seed=1)
            tr = MultimodalVAE(dict(cfg, lr=1e-3), feature_dims=dims, device=DEV)
            tr.model.train()
            tr.configure_optimizers()
            if captured:
                tr.capture(data)
            else:      # the same two warm-up passes capture() runs
                tr._one = torch.ones((), device=DEV)
                ops.LincombRows.unit_seed_ptr = tr._one.data_ptr()
                for _ in range(2):
                    tr._fwd_bwd(data)
                    tr._finish_step()
                tr.flat.zero_grad()
            tr.model._rng_state[1:].zero_()
            for m in tr.model.modules():
                if isinstance(m, DropoutState):
                    m.state[1:].zero_()
            y = torch.randint(0, 4, (32, 2), generator=torch.Generator().manual_seed(1))
            losses = []
            for step in range(3):
                if captured:
                    losses.append(float(tr.fused_step()["loss"].detach()))
                else:
                    losses.append(float(tr._fwd_bwd(data)["loss"].detach()))
                    tr.optimizer.step()
                    tr._finish_step()
                    tr.flat.zero_grad()
                if evaluate and step < 2:
                    tr.model.eval()
                    out = tr.classify_latents([(data, y)], [(data, y)], 4, epochs=2, batch_size=8)
                    tr.model.train()
                    assert len(out["accuracy"]) == 6 and bool(torch.isfinite(out["train_loss"]).all())
            torch.cuda.synchronize()
            opt = tr.optimizer
            res.append((losses, tr.flat.data.clone(), opt.m.clone(), opt.v.clone(), int(opt.step_dev[0])))
            del tr
    finally:
        DropoutState._next_seed[0] = seed0
        ops.LincombRows.unit_seed_ptr = None
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert res[0][4] == res[1][4] == 3
    for k, what in ((1, "parameters"), (2, "exp_avg"), (3, "exp_avg_sq")):
        bad = (res[0][k] != res[1][k]).nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} elements differ, first at {bad[:4].tolist()}"


# ---------------------------------------------------------------------------------------------
# 9. end to end
# ---------------------------------------------------------------------------------------------
E2E_LR, E2E_EPOCHS, E2E_BATCH = 0.05, 30, 64


def test_classify_latents_end_to_end(hip_lib):
    """a small MoPoE on synthetic CdSprites+ batches.  The latents are drawn by the generator (no eps_override) once, from
    a pinned evaluation state, and frozen: classify_latents, started from the same state, draws the same ones.  Column 0
    = argmax of the first 4 dimensions of the joint z (learnable: the restatement must reach 0.9 on the joint subset),
    column 1 random.  Every (subset, column): the restatement's accuracy under the rule of section 5, its mean test
    loss to 1e-5.  lr 0.05 (the argument, not the default): 240 Adam steps of 1e-3 cannot move a weight by more than
    0.24, too little to separate latents of this scale."""
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    tr, _ = _model("mopoe", D=16, B=64)
    model = tr.model
    names = list(model.vaes.keys())
    train_b = [_to_dev(cdsprites_batch(64, 8, seed=10 + i)) for i in range(8)]
    test_b = [_to_dev(cdsprites_batch(64, 8, seed=50 + i)) for i in range(4)]
    given = model.default_given()
    pinned = torch.tensor([4242, 0, 0], dtype=torch.int32)
    model._eval_rng_state.copy_(pinned)
    z_tr = [torch.cat([model.latents_for(b, g) for b in train_b]).cpu() for g in given]      # classify_latents' order
    z_te = [torch.cat([model.latents_for(b, g) for b in test_b]).cpu() for g in given]
    gen = torch.Generator().manual_seed(3)
    y_tr = torch.stack([z_tr[-1][:, :4].argmax(1), torch.randint(0, 5, (z_tr[-1].shape[0],), generator=gen)], 1)
    y_te = torch.stack([z_te[-1][:, :4].argmax(1), torch.randint(0, 5, (z_te[-1].shape[0],), generator=gen)], 1)
    n_classes = [4, 5]
    B = 64
    train = [(b, y_tr[i * B:(i + 1) * B]) for i, b in enumerate(train_b)]
    test = [(b, y_te[i * B:(i + 1) * B]) for i, b in enumerate(test_b)]
    model._eval_rng_state.copy_(pinned)
    train_state = model._rng_state.clone()
    out = tr.classify_latents(train, test, n_classes, epochs=E2E_EPOCHS, batch_size=E2E_BATCH, lr=E2E_LR, seed=5)
    torch.cuda.synchronize()
    assert torch.equal(model._rng_state, train_state)
    assert out["probes"] == [(s, a, n_classes[a]) for s in range(3) for a in range(2)]
    assert out["train_loss"].shape == (6, E2E_EPOCHS * 8)
    from multimodal_vae_comparison_amd import ops
    st0 = ops.probe_state(6, 16, 5, "cpu", seed=5)
    for p, (s, a, C) in enumerate(out["probes"]):
        key = ("+".join(given[s]), a)
        W0, b0 = ops.probe_weights(st0, p, C)
        ref = _ref_train(z_tr[s], y_tr[:, a], W0, b0, E2E_BATCH, E2E_EPOCHS, E2E_LR)
        with torch.no_grad():
            logits = ref["lin"](z_te[s].double())
        ref_loss = float(torch.nn.functional.cross_entropy(logits, y_te[:, a]))
        ref_pred = logits.argmax(1)
        ref_acc = float((ref_pred == y_te[:, a]).double().mean())
        print(f"{key}: accuracy {out['accuracy'][key]:.4f} (float64 {ref_acc:.4f}), loss {out['loss'][key]:.6f} "
              f"(float64 {ref_loss:.6f}), |z| max {float(z_tr[s].abs().max()):.3f}")
        if s == 2 and a == 0:
            assert ref_acc >= 0.9, f"the learnable column must be learnt by the restatement: {ref_acc}"
        check(out["train_loss"][p], ref["loss"], 1e-5, f"{key} loss curve")
        r32 = _ref_train(z_tr[s], y_tr[:, a], W0, b0, E2E_BATCH, E2E_EPOCHS, E2E_LR, dtype=torch.float32)
        with torch.no_grad():
            n32 = int((r32["lin"](z_te[s]).argmax(1) != ref_pred).sum())
        print(f"{key}: fp32 CPU restatement flips {n32} predictions")
        assert n32 == 0, (key, n32)
        bad = (out["pred"][key].long() != ref_pred).nonzero().flatten()
        top2 = logits.topk(2, 1).values
        gap = (top2[:, 0] - top2[:, 1])[bad]
        lim = 1e-5 * float(logits.abs().max())
        assert bad.numel() <= 2 and bool((gap <= lim).all()), (key, bad.tolist(), gap.tolist(), lim)
        assert abs(out["accuracy"][key] - ref_acc) <= bad.numel() / float(y_te.shape[0]) + 1e-12
        assert abs(out["loss"][key] - ref_loss) <= 1e-5 * max(abs(ref_loss), 1e-30), (key, out["loss"][key], ref_loss)
        assert torch.equal(tr.logged[f"test_latent_acc_{key[0]}_{a}"], torch.tensor(out["accuracy"][key], dtype=F64))
