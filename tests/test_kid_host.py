"""Host checks of the kernel inception distance.  The extended-precision restatement the GPU tests
of csrc/kid.hip are held to (tests/kid_reference.py) against a plain double loop and against an integer case worked by
hand; the condition on the seeded inputs; the plan and workspace queries of the library (pure host functions); what
kernel_distances and the ops refuse before anything reaches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

import kid_reference as K
from conftest import ROOT

SYMBOLS = ("mmvae_kid_chunks", "mmvae_kid_ws_doubles", "mmvae_kid_sums")


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------
def test_reference_against_a_plain_double_loop():
    X, Y, ix, iy, ref, bars = K.case(0)
    F, m = X.shape[1], ix.shape[1]
    for s in range(len(ix)):
        sxx = syy = sxy = 0.0
        for i in range(m):
            for j in range(m):
                for A, ia, B, jb, diagonal in ((X, ix, X, ix, False), (Y, iy, Y, iy, False), (X, ix, Y, iy, True)):
                    if i == j and not diagonal:
                        continue
                    dot = 0.0
                    for f in range(F):
                        dot += float(A[ia[s, i], f]) * float(B[jb[s, j], f])
                    t = dot / F + 1.0
                    v = t * t * t
                    if A is X and B is X:
                        sxx += v
                    elif A is Y and B is Y:
                        syy += v
                    else:
                        sxy += v
        got = np.array([sxx, syy, sxy])
        assert np.all(np.abs(got - ref["sums"][s].astype(np.float64)) <= bars["sum"]), (s, got, ref["sums"][s])
        mmd = sxx / (m * (m - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (m * m)
        assert abs(mmd - float(ref["mmd2"][s])) <= bars["mmd"]
    assert ref["m"] == m == 4 and ref["sums"].dtype == np.longdouble
    v = ref["mmd2"].astype(np.float64)
    assert abs(float(ref["kid"]) - v.mean()) <= 4 * K.U * np.abs(v).max() and abs(float(ref["std"]) - v.std()) <= 1e-15


def test_integer_case_by_hand():
    """k = (x . y / 2 + 1)^3 on even integer coordinates.  Subset 0 of the real rows: (0,0) (2,0) (0,2) (2,2) (4,2).
    (0,0) gives t = 1 with the four others: 4.  (2,0).(0,2) = 0: 1;  (2,0).(2,2) = 4: 3^3 = 27;  (2,0).(4,2) = 8: 5^3 = 125;
    (0,2).(2,2) = 4: 27;  (0,2).(4,2) = 4: 27;  (2,2).(4,2) = 12: 7^3 = 343.  Unordered 554, ordered i != j: 1108.
    The row (2,0) is in both sets: in sxy it meets itself (t = 3, 27) as an ordinary pair."""
    ix, iy = K.INT_IDX
    assert (K.INT_REAL % 2 == 0).all() and (K.INT_FAKE % 2 == 0).all()
    assert K.INT_REAL[1].tolist() == K.INT_FAKE[0].tolist() == [2, 0]
    ref = K.kid(K.INT_REAL, K.INT_FAKE, 2, 5, idx=K.INT_IDX, **K.INT_KERNEL)

    def k(a, b):
        t = (int(a[0]) * int(b[0]) + int(a[1]) * int(b[1])) // 2 + 1
        return t * t * t

    want = []
    for s in range(2):
        Xs, Ys = K.INT_REAL[ix[s]], K.INT_FAKE[iy[s]]
        want.append([sum(k(Xs[i], Xs[j]) for i in range(5) for j in range(5) if i != j),
                     sum(k(Ys[i], Ys[j]) for i in range(5) for j in range(5) if i != j),
                     sum(k(Xs[i], Ys[j]) for i in range(5) for j in range(5))])
    assert want == [[1108, 31140, 10641], [3548, 10668, 11449]]
    assert np.array_equal(ref["sums"], np.array(want, dtype=np.longdouble))
    # mmd2 = (sxx + syy) / 20 - 2 sxy / 25 = (5 (sxx + syy) - 8 sxy) / 100: 761.12 and -205.12 (a negative estimate)
    assert [5 * (w[0] + w[1]) - 8 * w[2] for w in want] == [76112, -20512]
    assert all(abs(float(v) - e) <= 1e-15 * abs(e) for v, e in zip(ref["mmd2"], (761.12, -205.12)))


def test_the_diagonal_is_a_matter_of_position():
    """a list that repeats a row number: only i == j is left out, the repeated row meets its copy as an ordinary pair"""
    X, Y, ix, iy, _, _ = K.case(0)
    rep = np.array(ix[:1])
    rep[0, 2] = rep[0, 0]
    got = K.sums(X, Y, rep, iy[:1])[0, 0]
    Xs = X[rep[0]]
    Kxx = K.gram(Xs, Xs, 3, 1.0 / X.shape[1], 1.0)
    assert got == Kxx.sum() - np.trace(Kxx) and Kxx[0, 2] == Kxx[0, 0]
    same = K.sums(X, X, ix, ix)
    diag = np.array([np.trace(K.gram(X[i], X[i], 3, 1.0 / X.shape[1], 1.0)) for i in ix])
    assert np.all(np.abs(same[:, 2] - (same[:, 0] + diag)) <= 1e-17 * np.abs(same[:, 2]))


def test_draw_is_the_documented_one():
    from multimodal_vae_comparison_amd import ops
    rs = np.random.RandomState(K.SEED)
    a0 = rs.choice(9, 4, replace=False)
    b0 = rs.choice(6, 4, replace=False)
    a1 = rs.choice(9, 4, replace=False)
    ia, ib = K.draw(9, 6, 3, 4)
    assert np.array_equal(ia[0], a0) and np.array_equal(ib[0], b0) and np.array_equal(ia[1], a1)
    assert ia.shape == ib.shape == (3, 4) and all(len(set(r)) == 4 for r in ia.tolist() + ib.tolist())
    oa, ob = ops.kid_draw(9, 6, 3, 4, K.SEED)
    assert np.array_equal(oa, ia) and np.array_equal(ob, ib)


@pytest.mark.parametrize("i", range(len(K.SHAPES)))
def test_inputs_make_the_bounds_a_demand(i):
    """every reference |mmd2| is at least 10^6 rounding bars (K.case asserts it; printed here), the same-distribution
    case holds negative estimates, every other case is clearly positive in the mean"""
    _, _, ix, _, ref, bars = K.case(i)
    v = ref["mmd2"].astype(np.float64)
    print(f"{K.SHAPES[i]}: mmd2 {v}, kid {float(ref['kid']):.4g} +- {float(ref['std']):.3g}, smallest |mmd2| = "
          f"{np.abs(v).min() / bars['mmd']:.3g} bars (bar {bars['mmd']:.3e})")
    assert np.abs(v).min() >= 1e6 * bars["mmd"] and ix.shape == (K.SHAPES[i][4], K.SHAPES[i][3])
    if i == K.SAME:
        assert int((v < 0).sum()) == 2 and abs(float(ref["kid"])) < float(ref["std"])
    else:
        assert float(ref["kid"]) > 0.0


# ---- 2. ABI and the plan -------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_header_and_the_ctypes_table():
    from multimodal_vae_comparison_amd import hipops
    src = open(os.path.join(ROOT, "include", "mmvae_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mmvae_hip.h"
        assert name in hipops.SIGNATURES, f"{name} is not in the ctypes table"
    for macro, value in (("MMVAE_KID_MAX_SUBSET", hipops.KID_MAX_SUBSET), ("MMVAE_KID_MAX_SUBSETS", hipops.KID_MAX_SUBSETS),
                         ("MMVAE_KID_MAX_DEGREE", hipops.KID_MAX_DEGREE)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    assert (hipops.KID_MAX_SUBSET, hipops.KID_MAX_SUBSETS, hipops.KID_MAX_DEGREE) == (16384, 1024, 8)


def test_plan_and_workspace_queries():
    from multimodal_vae_comparison_amd import hipops
    L = hipops.lib()
    # the default plan: min(ceil(512 / (3 S tiles)), ceil(tiles / 4)) chunks, tiles = ceil(m / 64), none of them empty
    assert L.mmvae_kid_chunks(100, 1000) == 1 and L.mmvae_kid_chunks(3, 4) == 1 and L.mmvae_kid_chunks(1024, 16384) == 1
    assert L.mmvae_kid_chunks(1, 1000) == 4      # 16 tiles: ceil(512 / 48) = 11, at least 4 tiles per chunk -> 4
    assert L.mmvae_kid_chunks(4, 300) == 2       # 5 tiles: ceil(512 / 60) = 9, ceil(5 / 4) = 2 -> chunks of 3 tiles
    assert L.mmvae_kid_chunks(2, 1000) == 4 and L.mmvae_kid_chunks(3, 1000) == 4 and L.mmvae_kid_chunks(11, 1000) == 1
    assert L.mmvae_kid_ws_doubles(100, 1000, 0) == 3 * 100 * 1000
    assert L.mmvae_kid_ws_doubles(4, 300, 0) == 3 * 4 * 2 * 300 and L.mmvae_kid_ws_doubles(4, 300, 1) == 3 * 4 * 300
    assert L.mmvae_kid_ws_doubles(4, 300, 5) == 3 * 4 * 5 * 300 and L.mmvae_kid_ws_doubles(4, 300, 99) == 3 * 4 * 5 * 300
    assert L.mmvae_kid_ws_doubles(4, 300, 4) == 3 * 4 * 3 * 300      # 5 tiles in chunks of 2: the fourth would be empty
    assert L.mmvae_kid_ws_doubles(1024, 16384, 1) == 3 * 1024 * 16384
    for S, m, chunks in ((0, 5, 0), (1025, 5, 0), (1, 1, 0), (1, 16385, 0), (1, 5, -1), (-1, 5, 0), (1, 0, 0)):
        assert L.mmvae_kid_ws_doubles(S, m, chunks) == 0
    assert L.mmvae_kid_chunks(0, 5) == 0 and L.mmvae_kid_chunks(1, 1) == 0 and L.mmvae_kid_chunks(1, 16385) == 0
    assert L.mmvae_kid_chunks(1025, 5) == 0


# ---- 3. refusals before a kernel -----------------------------------------------------------------------------------------------------
def _model(mixing="mopoe", mods=None, D=8):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, config_from_mods
    cfg, dims = config_from_mods(mixing, CD_MODS if mods is None else mods, D, batch_size=4)
    model = MultimodalVAE(cfg, feature_dims=dims, device="cpu").model
    model.eval()
    return model


def _flat(x):
    return x.float().reshape(x.shape[0], -1)[:, :4]


def test_unimodal_vae_refuses_kernel_distances_by_name():
    from multimodal_vae_comparison_amd.models.vae import VAE
    from multimodal_vae_comparison_amd.synthetic import CD_MODS
    vae = _model(mods=CD_MODS[:1])
    assert isinstance(vae, VAE)
    with pytest.raises(NotImplementedError) as e:
        vae.kernel_distances()
    assert "unimodal" in str(e.value) and "TorchMMVAE.kernel_distances" in str(e.value)


def test_train_mode_raises():
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch
    model = _model()
    model.train()
    with pytest.raises(RuntimeError, match="kernel_distances needs eval mode"):
        model.kernel_distances([cdsprites_batch(4, 6, seed=3)], {"mod_1": _flat})


def test_argument_errors_come_before_the_first_forward(monkeypatch):
    from multimodal_vae_comparison_amd.synthetic import CD_MODS, cdsprites_batch
    model = _model()
    batch = cdsprites_batch(4, 6, seed=3)
    calls = []
    forward = model.forward
    monkeypatch.setattr(model, "forward", lambda *a, **kw: calls.append(1) or forward(*a, **kw))
    with pytest.raises(ValueError, match="kernel_distances: `batches` is empty"):
        model.kernel_distances([], {"mod_1": _flat})
    with pytest.raises(ValueError, match="kernel_distances: .*callables"):
        model.kernel_distances([batch], {"mod_9": _flat})
    one = {m: dict(v, data=v["data"][:1], masks=None if v["masks"] is None else v["masks"][:1]) for m, v in batch.items()}
    with pytest.raises(ValueError, match="kernel_distances: 1 real rows, n_joint = 0"):
        model.kernel_distances([one], {"mod_1": _flat})
    with pytest.raises(ValueError, match="kernel_distances: 4 real rows, n_joint = 1"):
        model.kernel_distances([batch], {"mod_1": _flat}, n_joint=1)
    for subsets, size in ((0, 4), (1025, 4), (3, 1)):
        with pytest.raises(ValueError, match=f"kernel_distances: {subsets} subsets of {size} rows"):
            model.kernel_distances([batch], {"mod_1": _flat}, subsets=subsets, subset_size=size)
    assert not calls
    private = _model("dmvae", mods=[dict(m, private=4) for m in CD_MODS])
    with pytest.raises(NotImplementedError, match="kernel_distances"):
        private.kernel_distances([batch], {"mod_1": _flat}, n_joint=8)


def test_ops_refuse_before_a_launch():
    """on CPU tensors: every refusal comes before the device is asked for"""
    from multimodal_vae_comparison_amd import ops
    x, y = torch.ones(6, 4), torch.ones(5, 4)
    ix, iy = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"kid_sums: X is \(6,\)"):
        ops.kid_sums(torch.ones(6), y, ix, iy)
    with pytest.raises(ValueError, match="kid_sums: Y is .*int64"):
        ops.kid_sums(x, torch.ones(5, 4, dtype=torch.int64), ix, iy)
    with pytest.raises(ValueError, match="kid_sums: X has F = 2049"):
        ops.kid_sums(torch.ones(6, 2049), torch.ones(5, 2049), ix, iy)
    with pytest.raises(ValueError, match="kid_sums: X has F = 4 features, Y F = 3"):
        ops.kid_sums(x, torch.ones(5, 3), ix, iy)
    with pytest.raises(ValueError, match="kid_sums: X is on cpu, Y on meta"):
        ops.kid_sums(x, torch.ones(5, 4, device="meta"), ix, iy)
    with pytest.raises(ValueError, match="kid_sums: Y holds values that are not finite"):
        ops.kid_sums(x, torch.full((5, 4), float("inf")), ix, iy)
    with pytest.raises(ValueError, match="kid_sums: idx_x is .*float32"):
        ops.kid_sums(x, y, ix.float(), iy)
    with pytest.raises(ValueError, match=r"kid_sums: idx_x is \(2, 3\), idx_y \(2, 4\)"):
        ops.kid_sums(x, y, ix, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"kid_sums: idx_x is \(3,\)"):
        ops.kid_sums(x, y, ix[0], iy[0])
    with pytest.raises(ValueError, match="kid_sums: idx_x is 2 subsets of m = 1 rows"):
        ops.kid_sums(x, y, ix[:, :1], iy[:, :1])
    with pytest.raises(ValueError, match="kid_sums: idx_x is 1025 subsets"):
        ops.kid_sums(x, y, torch.zeros(1025, 3, dtype=torch.int64), torch.zeros(1025, 3, dtype=torch.int64))
    bad = ix.clone()
    bad[1, 2] = -1
    with pytest.raises(ValueError, match="kid_sums: idx_x holds row numbers from -1 to 0; the set has the rows 0 .. 5"):
        ops.kid_sums(x, y, bad, iy)
    bad = iy.clone()
    bad[0, 1] = 5
    with pytest.raises(ValueError, match="kid_sums: idx_y holds row numbers from 0 to 5; the set has the rows 0 .. 4"):
        ops.kid_sums(x, y, ix, bad)
    for degree in (0, 9):
        with pytest.raises(ValueError, match=f"kid_sums: degree = {degree}"):
            ops.kid_sums(x, y, ix, iy, degree=degree)
    with pytest.raises(ValueError, match="kid_sums: chunks = -1"):
        ops.kid_sums(x, y, ix, iy, chunks=-1)
    with pytest.raises(ValueError, match="kid_sums: gamma = nan"):
        ops.kid_sums(x, y, ix, iy, gamma=float("nan"))
    with pytest.raises(ValueError, match="kid_sums: X is on cpu; the kernel runs on the MI355X"):
        ops.kid_sums(x, y, ix, iy)
    who = "kernel_inception_distance"
    with pytest.raises(ValueError, match=f"{who}: m = .* = 1 "):
        ops.kernel_inception_distance(x, torch.ones(1, 4))
    with pytest.raises(ValueError, match=f"{who}: m = .* = 1 "):
        ops.kernel_inception_distance(x, y, subset_size=1)
    with pytest.raises(ValueError, match=f"{who}: 0 subsets of m = 5 rows"):
        ops.kernel_inception_distance(x, y, subsets=0)
    with pytest.raises(ValueError, match=f"{who}: idx_real is 2 subsets of m = 1 rows"):
        ops.kernel_inception_distance(x, y, idx=(ix[:, :1], iy[:, :1]))
    with pytest.raises(ValueError, match=f"{who}: idx_fake holds row numbers from 0 to 5"):
        ops.kernel_inception_distance(x, y, idx=(ix, bad))
    with pytest.raises(ValueError, match=f"{who}: real has F = 4 features, fake F = 3"):
        ops.kernel_inception_distance(x, torch.ones(5, 3))
    with pytest.raises(ValueError, match=f"{who}: real is on cpu; the kernel runs on the MI355X"):
        ops.kernel_inception_distance(x, y, subsets=2)
