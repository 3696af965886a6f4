"""The float64 references of tests/optim_reference.py are what they claim to be, and their error bounds hold for a correct
fp32 update that is NOT the code under test (the numpy emulation in the same module).  No GPU, no library call."""
import numpy as np
import pytest
import torch

import optim_reference as R

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
GSCALES = (1.0, 0.5, 1.0 / 3.0)
SIZES = (1, 3, 4, 5, 1023, 10007, 4202499)


def test_adam_reference_is_torch_adam_amsgrad_in_float64():
    """6 steps against torch.optim.Adam(amsgrad=True) in float64 with betas = (float32(0.9), float32(0.999)); step 3 has a
    100x gradient, so vmax > v afterwards: p, exp_avg, exp_avg_sq, max_exp_avg_sq to 1e-12"""
    rng = np.random.default_rng(3)
    n = 257
    lr, eps = R.f32(LR), R.f32(EPS)
    p0 = rng.standard_normal(n).astype(np.float32)
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(R.f32(B1), R.f32(B2)), eps=eps, amsgrad=True)
    p, m, v, x = p0.astype(np.float64), np.zeros(n), np.zeros(n), np.zeros(n)
    for step in range(1, 7):
        g = (rng.standard_normal(n) * (10.0 if step == 3 else 0.1)).astype(np.float32)
        pt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, m, v, x = R.adam_amsgrad_step(p, g, m, v, x, LR, B1, B2, EPS, step, 1.0)
        st = opt.state[pt]
        for name, mine, theirs in (("p", p, pt.detach()), ("exp_avg", m, st["exp_avg"]), ("exp_avg_sq", v, st["exp_avg_sq"]),
                                   ("max_exp_avg_sq", x, st["max_exp_avg_sq"])):
            theirs = theirs.numpy()
            err = np.abs(mine - theirs).max() / max(np.abs(theirs).max(), 1e-300)
            assert err <= 1e-12, f"step {step} {name}: {err:.3e}"
    assert (x > v).mean() > 0.5          # the large step left the running maximum above v


def test_adam_reference_applies_grad_scale_to_the_gradient():
    p, g, m, v, x = R.adam_case(101, "mid")
    a = R.adam_amsgrad_step(p, g, m, v, x, LR, B1, B2, EPS, 7, 0.5)
    b = R.adam_amsgrad_step(p, (g.astype(np.float64) * 0.5), m, v, x, LR, B1, B2, EPS, 7, 1.0)
    for q, r in zip(a, b):
        assert np.array_equal(q, r)


def test_adabelief_reference_is_the_oracle():
    """oracle.mmvae_oracle.adabelief_step on a small dict, run in float64 over 4 steps.  The precision that function
    allows is set by its constants, not by its arithmetic: it uses ONE double beta for decay, gain (1 - beta) and bias
    correction, the kernel's convention (this reference) a decay float32(beta) and a gain float32(1 - beta).  With the double
    betas the decays differ by 2.4e-8 / 1.3e-8 relative and bc2 = 1 - beta2^step at step 1 by 1.3e-8 / 1e-3 = 1.3e-5; with
    the fp32-rounded betas the gain 1 - float32(0.999) differs from float32(0.001) by 1.3e-5 instead.  Either way 1.3e-5
    relative is the floor: checked at 2e-5 of each tensor's maximum, with both sets of betas."""
    from oracle import mmvae_oracle as orc
    rng = np.random.default_rng(5)
    shapes = {"w": (7, 5), "b": (11,)}
    lr, eps = R.f32(LR), R.f32(1e-16)
    for b1, b2, tol in ((B1, B2, 2e-5), (R.f32(B1), R.f32(B2), 2e-5)):
        params = {k: torch.tensor(rng.standard_normal(s).astype(np.float32), dtype=torch.float64) for k, s in shapes.items()}
        state = {k: (torch.zeros(s, dtype=torch.float64), torch.zeros(s, dtype=torch.float64)) for k, s in shapes.items()}
        mine = {k: (params[k].numpy().copy(), np.zeros(s), np.zeros(s)) for k, s in shapes.items()}
        for step in range(1, 5):
            grads = {k: torch.tensor(rng.standard_normal(s).astype(np.float32) * 0.1, dtype=torch.float64)
                     for k, s in shapes.items()}
            orc.adabelief_step(params, grads, state, lr, step, b1=b1, b2=b2, eps=eps)
            for k in shapes:
                p, m, s_ = mine[k]
                mine[k] = R.adabelief_step(p, grads[k].numpy(), m, s_, LR, B1, B2, 1e-16, step, 1.0)
                for name, a, b in (("p", mine[k][0], params[k]), ("m", mine[k][1], state[k][0]), ("s", mine[k][2], state[k][1])):
                    b = b.numpy()
                    err = np.abs(a - b).max() / np.abs(b).max()
                    assert err <= tol, f"betas {b1, b2} step {step} {k}.{name}: {err:.3e} > {tol}"


def _worst(res, ref, bound, scale, units):
    err = np.abs(res.astype(np.float64) - ref)
    bad = ~(err <= bound)
    assert not bad.any(), f"{int(bad.sum())} elements outside the bound, first {np.flatnonzero(bad)[:5].tolist()}, " \
                          f"err {err[bad][:3]}, bound {bound[bad][:3]}"
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(scale > 0, err / (scale * units), 0.0)))


def test_fp32_emulation_of_adam_stays_inside_the_bounds(capsys):
    worst = {"m": 0.0, "v": 0.0, "vmax": 0.0, "p": 0.0}
    for n in SIZES:
        combos = [("mid", 1.0 / 3.0, 42), ("zero", 0.5, 1)] if n > 100000 else [
            (st, gs, step) for st in ("zero", "mid") for gs in GSCALES for step in ((1,) if st == "zero" else (7, 42, 43))]
        for st, gs, step in combos:
            p, g, m, v, x = R.adam_case(n, st)
            ref = R.adam_amsgrad_step(p, g, m, v, x, LR, B1, B2, EPS, step, gs)
            bd = R.adam_bounds(p, g, m, v, x, LR, B1, B2, EPS, step, gs)
            P, M, V, X = R.emulate_adam(p, g, m, v, x, LR, B1, B2, EPS, step, gs)
            assert np.array_equal(X, np.maximum(x, V))
            worst["m"] = max(worst["m"], _worst(M, ref[1], bd["m"], bd["Tm"], R.U))
            worst["v"] = max(worst["v"], _worst(V, ref[2], bd["v"], bd["Tv"], R.U))
            worst["vmax"] = max(worst["vmax"], _worst(X, ref[3], bd["vmax"], ref[3], R.U))
            half = 0.5 * R.ulp32(np.maximum(np.abs(p.astype(np.float64)), np.abs(ref[0])))
            _worst(P, ref[0], bd["p"], bd["S"], R.U)
            over = np.maximum(np.abs(P.astype(np.float64) - ref[0]) - half, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst["p"] = max(worst["p"], float(np.nanmax(np.where(bd["S"] > 0, over / (bd["S"] * R.U), 0.0))))
    with capsys.disabled():
        print("\nemulated Adam, maxima in u of the term scale: " + ", ".join(f"{k} {w:.2f}" for k, w in worst.items()))
    assert worst["m"] <= 3 and worst["v"] <= 5 and worst["vmax"] <= 5 and worst["p"] <= 12


@pytest.mark.parametrize("gval", [0.0, 1e-20, 1e15])
def test_fp32_emulation_of_adam_edge_gradients(gval, capsys):
    n = 64
    p, _, m, v, x = R.adam_case(n, "zero")
    g = np.full(n, gval, np.float32)
    ref = R.adam_amsgrad_step(p, g, m, v, x, LR, B1, B2, EPS, 1, 1.0)
    bd = R.adam_bounds(p, g, m, v, x, LR, B1, B2, EPS, 1, 1.0)
    P, M, V, X = R.emulate_adam(p, g, m, v, x, LR, B1, B2, EPS, 1, 1.0)
    assert all(np.isfinite(a).all() for a in (P, M, V, X))
    for res, rf, b in ((P, ref[0], bd["p"]), (M, ref[1], bd["m"]), (V, ref[2], bd["v"]), (X, ref[3], bd["vmax"])):
        assert (np.abs(res.astype(np.float64) - rf) <= b).all()
    if gval == 0.0:
        assert np.array_equal(P, p) and not M.any() and not V.any()
    if gval == 1e-20:      # why the bounds carry an absolute floor: v is subnormal, 5u of it cannot hold
        rel = float((np.abs(V.astype(np.float64) - ref[2]) / (bd["Tv"] * R.U)).max())
        with capsys.disabled():
            print(f"\nemulated v at g = 1e-20: {rel:.3g} u of Tv (subnormal result)")
        assert rel > 5


def test_fp32_emulation_of_adabelief_stays_inside_the_bounds(capsys):
    worst = {"m": 0.0, "s": 0.0, "p": 0.0}
    for n in (1, 5, 10007, 2100003):
        combos = [("mid", 1.0 / 3.0, 42)] if n > 100000 else [(st, gs, step) for st in ("zero", "mid") for gs in GSCALES
                                                              for step in ((1,) if st == "zero" else (7, 42, 43))]
        for st, gs, step in combos:
            p, g, m, s = R.belief_case(n, st)
            ref = R.adabelief_step(p, g, m, s, LR, B1, B2, 1e-16, step, gs)
            bd = R.adabelief_bounds(p, g, m, s, LR, B1, B2, 1e-16, step, gs)
            P, M, S = R.emulate_adabelief(p, g, m, s, LR, B1, B2, 1e-16, step, gs)
            worst["m"] = max(worst["m"], _worst(M, ref[1], bd["m"], bd["Tm"], R.U))
            worst["s"] = max(worst["s"], _worst(S, ref[2], bd["s"], bd["s"], 1.0))
            _worst(P, ref[0], bd["p"], bd["p"], 1.0)
            half = 0.5 * R.ulp32(np.maximum(np.abs(p.astype(np.float64)), np.abs(ref[0])))
            over = np.maximum(np.abs(P.astype(np.float64) - ref[0]) - half, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst["p"] = max(worst["p"], float(np.nanmax(np.where(bd["p_rel"] > 0, over / bd["p_rel"], 0.0))))
    with capsys.disabled():
        print(f"\nemulated AdaBelief: m {worst['m']:.2f} u of Tm, s {worst['s']:.2f} of its bound, p - 1/2 ulp {worst['p']:.2f} of the rest of its bound")
    assert worst["m"] <= 3


def test_fp32_emulation_of_fold_then_adam_stays_inside_the_propagated_bounds(capsys):
    """a gradient that is itself an fp32 sum (rows added one by one onto the direct contribution, the worst order for the
    bound) through the emulated update: inside adam_bounds(..., g_err = the fold's bound)"""
    rng = np.random.default_rng(9)
    n = 3000
    p, g, m, v, x = R.adam_case(n, "mid", seed=7)
    g = g * (rng.random(n) < 0.5).astype(np.float32)
    segs, so = [], 0
    for do, rows, ln in ((0, 33, 256), (257, 130, 77), (257, 5, 77), (400, 1, 1), (1000, 512, 257), (n - 13, 9, 13)):
        segs.append((so, do, rows, ln, ln + 3))
        so += rows * (ln + 3)
    arena = rng.standard_normal(so, dtype=np.float32)
    gfold, gerr = R.fold(g, arena, segs)
    g32 = g.copy()
    for so, do, rows, ln, sd in segs:
        for r in range(rows):
            g32[do:do + ln] += arena[so + r * sd:so + r * sd + ln]
    assert (np.abs(g32.astype(np.float64) - gfold) <= gerr).all() and (gerr[500:900] == 0).all()
    worst = {}
    for gs in (0.5, 1.0 / 3.0):
        ref = R.adam_amsgrad_step(p, gfold, m, v, x, LR, B1, B2, EPS, 42, gs)
        bd = R.adam_bounds(p, gfold, m, v, x, LR, B1, B2, EPS, 42, gs, g_err=gerr)
        out = R.emulate_adam(p, g32, m, v, x, LR, B1, B2, EPS, 42, gs)
        for name, res, rf in zip(("p", "m", "v", "vmax"), out, ref):
            worst[name] = max(worst.get(name, 0.0), _worst(res, rf, bd[name], bd[name], 1.0))
    with capsys.disabled():
        print("\nemulated fold + Adam, fraction of the propagated bound: " + ", ".join(f"{k} {w:.2f}" for k, w in worst.items()))


def test_fold_and_rider_references():
    arena = np.arange(200, dtype=np.float32)
    dst = np.ones(20, np.float32)
    # two segments chained onto elements 2..5, one onto 10..12; stride > len
    out, bound = R.fold(dst, arena, [(0, 2, 3, 4, 10), (100, 2, 2, 4, 7), (50, 10, 1, 3, 3)])
    exp = np.ones(20)
    for i in range(4):
        exp[2 + i] += (0 + i) + (10 + i) + (20 + i) + (100 + i) + (107 + i)
    exp[10:13] += [50, 51, 52]
    assert np.array_equal(out, exp)
    assert bound[0] == 0 and bound[13] == 0 and bound[2] == (5 + 2) * R.U * exp[2] + R.TINY
    o, b = R.rider([[1.0, 2.0], [0.0, -1.0]], np.array([[1.0, 2.0, 3.0], [4.0, 5.0, -6.0]]))
    assert np.array_equal(o, [6 + 2 * 3, -3.0]) and b[0] == (3 + 2 + 3) * R.U * (6 + 2 * 15) + R.TINY
