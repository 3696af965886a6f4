"""The batched ConvTranspose2d weight-gradient launch (mmvae_conv_wgrad_batch, csrc/conv.hip) against the fused backward
launches whose weight-gradient halves it takes over (mmvae_convT2d_k4s2_bwd): every comparison is bit for bit -- the same
conv_wgrad_body instantiation walks the same macro tiles in the same order, only the launch it sits in differs -- and so is
the captured cfg2 step with the image decoder's two large weight gradients parked (ops.GradReducer.cw_later)."""
import ctypes

import pytest
import torch

DEV = "cuda"
# Dec_CNN's last two layers (models/decoders.py:62-69): (Cin, Cout, Hin, activation of the layer's input)
T3 = (32, 3, 32)
T2 = (32, 32, 16)
# 64: the smallest batch at which the 32 -> 32 layer's data gradient takes the split-bf16 gather body (8 B >= 512 tiles);
# 20: not a power of two, the 32 -> 3 layer below ITS split-bf16 threshold (32 B >= 1024), short splits; 128: the benchmark's
BATCHES = (20, 64, 128)


def _layout(lib, B, geom):
    Cin, Cout, Hin = geom
    rows, rowlen, bias_col = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.mmvae_conv_wgrad_layout(B, Cin, Cout, Hin, ctypes.byref(rows), ctypes.byref(rowlen), ctypes.byref(bias_col)) == 0
    return rows.value, rowlen.value, bias_col.value


def _spec(lib, B, geom):
    """(n_macro, nsplit, long-split loop form?) of the layer's weight gradient, from the library's layout query:
    n_macro = ceil(B * Hin / (64 / Hin)) macro tiles of 64 positions; one partial row per split (two for the 3-channel
    layer, whose wave pairs split the positions); the specialised loops from 16 macro tiles per split on"""
    Cin, Cout, Hin = geom
    nrows = 64 // Hin
    n_macro = (B * Hin + nrows - 1) // nrows
    rows, _, _ = _layout(lib, B, geom)
    nsplit = rows // (1 if Cout >= 16 else 2)
    return n_macro, nsplit, n_macro >= 16 * nsplit


def test_split_plan_of_the_tested_batches():
    """the batches of the GPU tests below sit where they claim to: no batch takes the long-split (SPEC) loops, 20 is no
    multiple of anything in the tiling, and both layers have their full number of splits (256 / 64 workgroup columns)"""
    from multimodal_vae_comparison_amd import hipops
    lib = hipops.lib()
    for B in BATCHES:
        for geom, want in ((T3, 256), (T2, 64)):
            n_macro, nsplit, spec = _spec(lib, B, geom)
            assert nsplit == want and n_macro > nsplit and not spec, (B, geom, n_macro, nsplit, spec)
    assert _spec(lib, 20, T3)[0] % 256 and _spec(lib, 20, T2)[0] % 64      # ragged: splits of unequal length
    assert _spec(lib, 256, T3)[2] and _spec(lib, 256, T2)[2]                  # (where the other loop form starts)


_inputs = {}


def _layer(B, geom, act):
    """inputs of one layer and what its FUSED backward launch leaves: dx, raw partials (ACC_DEFER), dW, db; computed once"""
    from multimodal_vae_comparison_amd import hipops as H
    key = (B, geom, act)
    if key in _inputs:
        return _inputs[key]
    lib = H.lib()
    Cin, Cout, Hin = geom
    g = torch.Generator(device="cpu").manual_seed(1000 * B + Cout)
    x = torch.randn(B, Cin, Hin, Hin, generator=g).to(DEV)
    dy = torch.randn(B, Cout, 2 * Hin, 2 * Hin, generator=g).to(DEV)
    w = (0.1 * torch.randn(Cin, Cout, 4, 4, generator=g)).to(DEV)
    nws = lib.mmvae_conv_wgrad_ws_floats(B, Cin, Cout, Hin)
    rows, rowlen, _ = _layout(lib, B, geom)
    assert nws == rows * rowlen
    ws = torch.full((nws,), -7.0, device=DEV)      # (slots no workgroup writes keep the sentinel in both runs)
    dx = torch.full_like(x, float("nan"))
    dw, db = torch.empty_like(w), torch.empty(Cout, device=DEV)
    H.check(lib.mmvae_convT2d_k4s2_bwd(H.ptr(dy), H.ptr(x), H.ptr(w), H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(ws), B, Cin,
                                       Cout, Hin, act, H.ACC_DEFER, H.stream()), "bwd")
    ws2 = torch.full((nws,), -7.0, device=DEV)
    dx2 = torch.full_like(x, float("nan"))
    H.check(lib.mmvae_convT2d_k4s2_bwd(H.ptr(dy), H.ptr(x), H.ptr(w), H.ptr(dx2), H.ptr(dw), H.ptr(db), H.ptr(ws2), B, Cin,
                                       Cout, Hin, act, 0, H.stream()), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(ws, ws2) and torch.equal(dx, dx2)      # (the yardstick itself is reproducible)
    _inputs[key] = dict(x=x, dy=dy, w=w, dx=dx, ws=ws, dw=dw, db=db, geom=geom, act=act, B=B)
    return _inputs[key]


def _batch(layers):
    """the layers' weight gradients as ONE batched launch -> per layer (raw partials, dW, db)"""
    from multimodal_vae_comparison_amd import hipops as H
    lib = H.lib()
    arr = (H.ConvWgradJob * len(layers))()
    wss = []
    for j, L in zip(arr, layers):
        ws = torch.full_like(L["ws"], -7.0)
        wss.append(ws)
        Cin, Cout, Hin = L["geom"]
        j.x, j.dy, j.ws = H.ptr(L["x"]), H.ptr(L["dy"]), H.ptr(ws)
        j.B, j.Cin, j.Cout, j.Hin, j.x_act, j.has_bias = L["B"], Cin, Cout, Hin, L["act"], 1
    H.check(lib.mmvae_conv_wgrad_batch(ctypes.cast(arr, ctypes.c_void_p), len(layers), H.stream()), "batch")
    out = []
    for L, ws in zip(layers, wss):
        Cin, Cout, Hin = L["geom"]
        rows, rowlen, bias_col = _layout(lib, L["B"], L["geom"])
        dw, db = torch.empty_like(L["w"]), torch.empty(Cout, device=DEV)
        H.check(lib.mmvae_reduce_rows(H.ptr(ws), H.ptr(dw), rows, bias_col, rowlen, 0, H.stream()), "reduce")
        H.check(lib.mmvae_reduce_rows(ws.data_ptr() + 4 * bias_col, H.ptr(db), rows, Cout, rowlen, 0, H.stream()), "reduce")
        out.append((ws, dw, db))
    torch.cuda.synchronize()
    return out


def _same(got, L, what):
    ws, dw, db = got
    assert torch.equal(ws, L["ws"]), f"{what}: {int((ws != L['ws']).sum())} partials differ"
    assert torch.equal(dw, L["dw"]), f"{what}: dW differs"
    assert torch.equal(db, L["db"]), f"{what}: db differs"
    assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
def test_batched_weight_gradients_equal_the_fused_launches(hip_lib, B):
    """both jobs in one launch (the step's order: last layer first, its input SiLU-activated as in Dec_CNN): raw partial
    rows, dW and db of each layer bit-identical to its fused backward launch"""
    from multimodal_vae_comparison_amd import hipops as H
    l3, l2 = _layer(B, T3, H.ACT_SILU), _layer(B, T2, H.ACT_SILU)
    got = _batch([l3, l2])
    _same(got[0], l3, f"32->3, B={B}")
    _same(got[1], l2, f"32->32, B={B}")


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
def test_data_gradient_alone_equals_the_fused_launch(hip_lib, B):
    """mmvae_convT2d_k4s2_dgrad at the two shapes picks the body (split-bf16 gather from 32 resp. 64 images on, fp32 gather
    below) and tile order of the fused launch's data-gradient part: dx bit-identical"""
    from multimodal_vae_comparison_amd import hipops as H
    lib = H.lib()
    for geom in (T3, T2):
        L = _layer(B, geom, H.ACT_SILU)
        Cin, Cout, Hin = geom
        dx = torch.full_like(L["x"], float("nan"))
        H.check(lib.mmvae_convT2d_k4s2_dgrad(H.ptr(L["dy"]), H.ptr(L["w"]), H.ptr(L["x"]), H.ptr(dx), B, Cin, Cout, Hin,
                                             H.EP_MUL_SILU_GRAD, H.stream()), "dgrad")
        torch.cuda.synchronize()
        assert torch.isfinite(dx).all()
        assert torch.equal(dx, L["dx"]), (geom, B, int((dx != L["dx"]).sum()))


@pytest.mark.gpu
def test_one_job_and_mixed_batches(hip_lib):
    """a job alone, and the two geometries in either order (the job table's first workgroup and the launch's LDS size must
    not depend on which geometry comes first), jobs of different batch and activation side by side"""
    from multimodal_vae_comparison_amd import hipops as H
    l3, l2 = _layer(64, T3, H.ACT_SILU), _layer(64, T2, H.ACT_SILU)
    l3r, l2n = _layer(20, T3, H.ACT_RELU), _layer(20, T2, H.ACT_NONE)
    _same(_batch([l3])[0], l3, "32->3 alone")
    _same(_batch([l2])[0], l2, "32->32 alone")
    got = _batch([l2, l3])
    _same(got[0], l2, "32->32 first")
    _same(got[1], l3, "32->3 second")
    got = _batch([l3r, l2, l2n, l3])
    for g_, L, what in zip(got, (l3r, l2, l2n, l3), ("relu 32->3 B=20", "32->32 B=64", "plain 32->32 B=20", "32->3 B=64")):
        _same(g_, L, what)


@pytest.mark.gpu
def test_unsupported_jobs_are_refused(hip_lib):
    """no silent fallback: other geometries, jobs that need different loop forms, too many jobs"""
    from multimodal_vae_comparison_amd import hipops as H
    lib = H.lib()
    L = _layer(20, T2, H.ACT_NONE)

    def rc(jobs):
        arr = (H.ConvWgradJob * len(jobs))()
        for j, (geom, B) in zip(arr, jobs):
            j.x, j.dy, j.ws = H.ptr(L["x"]), H.ptr(L["dy"]), H.ptr(L["ws"])
            j.B, (j.Cin, j.Cout, j.Hin), j.x_act, j.has_bias = B, geom, H.ACT_NONE, 1
        return lib.mmvae_conv_wgrad_batch(ctypes.cast(arr, ctypes.c_void_p), len(jobs), H.stream())

    unsupported = rc([((32, 32, 8), 20)])
    assert unsupported != 0
    assert rc([((32, 3, 16), 20)]) == unsupported and rc([((64, 32, 16), 20)]) == unsupported
    assert rc([(T2, 20), (T2, 256)]) == unsupported               # short and long splits in one launch
    assert rc([(T2, 20)] * (H.CONV_WGRAD_BATCH_MAX + 1)) == unsupported
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [32, 128])
def test_parked_conv_weight_gradients_train_bit_identically(hip_lib, monkeypatch, B):
    """The captured one-GPU cfg2 step with the image decoder's large weight gradients parked (MMVAE_CONV_DW_LATER, the
    default; batch 32: both layers, batch 128: the last layer alone -- ops.GradReducer.CW_MAX_BATCH) against the same step
    with the fused backward launches: losses of three steps, parameters, both moments and the running maximum equal bit
    for bit; the parked plan has one launch more (n fused launches -> n data-gradient launches + the batch)."""
    from multimodal_vae_comparison_amd import ops
    from multimodal_vae_comparison_amd.models.nn_modules import DropoutState
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch, cdsprites_config
    batch = cdsprites_batch(B, 32, seed=2)
    batch = {k: {kk: (vv.to(DEV) if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in batch.items()}
    res = []
    seed0 = DropoutState._next_seed[0]
    try:
        for flag in (False, True):
            monkeypatch.setattr(ops.GradReducer, "cw_enabled", flag)
            torch.manual_seed(0)
            DropoutState._next_seed[0] = 0x1234567
            tr = MultimodalVAE(cdsprites_config("mopoe", 32, lr=1e-3), device=DEV)
            tr.model.train()
            tr.configure_optimizers()
            tr.capture({k: dict(v) for k, v in batch.items()})
            tr.model._rng_state[1:].zero_()
            for m in tr.model.modules():
                if isinstance(m, DropoutState):
                    m.state[1:].zero_()
            losses = [float(tr.fused_step()["loss"]) for _ in range(3)]
            torch.cuda.synchronize()
            opt = tr.optimizer
            res.append((losses, tr.flat.data.clone(), opt.m.clone(), opt.v.clone(), opt.vmax.clone(), tr.abi_calls_in_graph))
    finally:
        DropoutState._next_seed[0] = seed0
    assert ops.GradReducer.CW_MAX_BATCH == {(32, 3, 32): 128, (32, 32, 16): 64}
    assert res[1][5] == res[0][5] + 1, (res[0][5], res[1][5])
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for k, what in ((1, "parameters"), (2, "exp_avg"), (3, "exp_avg_sq"), (4, "max_exp_avg_sq")):
        assert torch.equal(res[0][k], res[1][k]), f"{what} differ: {int((res[0][k] != res[1][k]).sum())} elements"

