"""GPU parity of the latent-sampling family against float64 restatements: the MoE K-sample draw and its DReG / IWAE
losses (csrc/moe.hip), the MoE ELBO helpers (Laplace KL and importance ratios, csrc/moe.hip + csrc/latent.hip; expmul
and the ELBO assembly, csrc/loss.hip), and the device noise generators (mmvae_randn, mmvae_rand_laplace) as
distributions.  References: MOE.pz_params / objective / forward (models/mmvae_models.py:28-117),
MultimodalObjective.iwae / dreg (models/objectives.py:342-387), BaseObjective.elbo (objectives.py:54-67)."""
import ctypes
import itertools
import math

import pytest
import torch
import torch.nn.functional as F
from torch.distributions import Laplace, Normal, kl_divergence

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def check(a, b, tol, what):
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    e = rel_err(a, b)
    assert math.isfinite(e) and e <= tol, f"{what}: rel err {e:.3e} > {tol}"


def check_fp32_rounding(a, b, what):
    """every element of the fp32 result within one fp32 ulp of the float64 reference (kernels that compute in fp64 and
    round once)"""
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    bad = (a - b).abs() > 2.0 ** -23 * b.abs() + 1e-37
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off by more than an fp32 ulp, e.g. " \
                                f"{float(a[bad][0])} vs {float(b[bad][0])}"


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    return ops


@pytest.fixture(scope="module")
def H(hip_lib):
    from multimodal_vae_comparison_amd import hipops
    return hipops


def _laplace_eps(shape, g):
    """standard-Laplace variates by the inverse CDF (Laplace.rsample's construction), fp32"""
    u = torch.rand(shape, generator=g) * 1.999 - 0.9995
    return -(u.sign() * torch.log1p(-u.abs()))


def _dist(lap, mu, s):
    return Laplace(mu, s) if lap else Normal(mu, s)


# ---------------------------------------------------------------------------------------------
# MoE K-sample draw (ops.moe_ksample): z_r = mu_r + s_r eps_r,
#   lat[r,k,b] = sum_d log N(z; 0, D softmax theta) - beta log-mean-exp_m sum_d log q_m(z)
# (MOE.pz_params :28-30, MOE.forward :96-100, _m_dreg_looser objectives.py:366-373, iwae :352-356)
# ---------------------------------------------------------------------------------------------
def _ref_moe_ksample(theta, packed, eps, laplace, beta):
    """float64, autograd: -> lat (M,K,B), z (M,K,B,D), pi (M,K,B,M)"""
    M = len(packed)
    D = theta.shape[-1]
    sp = F.softmax(theta, -1) * D
    lats, zs, pis = [], [], []
    for r in range(M):
        z = packed[r][:, :D] + packed[r][:, D:] * eps[r]
        lpz = Normal(torch.zeros_like(sp), sp).log_prob(z).sum(-1)
        lq = torch.stack([_dist(laplace[m], packed[m][:, :D], packed[m][:, D:]).log_prob(z).sum(-1) for m in range(M)])
        lats.append(lpz - beta * (torch.logsumexp(lq, 0) - math.log(M)))
        zs.append(z)
        pis.append(torch.softmax(lq, 0).permute(1, 2, 0))
    return torch.stack(lats), torch.stack(zs), torch.stack(pis)


def _moe_inputs(M, K, B, D, laplace, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(B, D, generator=g)
    packed = [torch.cat([mu + 0.5 * torch.randn(B, D, generator=g), 0.5 + torch.rand(B, D, generator=g)], -1)
              for _ in range(M)]
    eps = [_laplace_eps((K, B, D), g) if laplace[m] else torch.randn(K, B, D, generator=g) for m in range(M)]
    theta = torch.randn(1, D, generator=g) * 0.3
    dlat = torch.randn(M, K, B, generator=g)
    dz = torch.randn(M, K, B, D, generator=g)
    return theta, packed, eps, dlat, dz


def _run_moe_ksample(ops, theta, packed, eps, laplace, beta, dlat, dz, mode, monkeypatch):
    """GPU forward + backward -> (lat, z, dpacked list, dtheta, pi).  mode: the theta gradient's form --
    'returned' (theta.grad), 'acc_off' (accumulated into a preset gtheta, GradReducer off), 'acc_on' (the same through
    GradReducer's deferred partials, folded by the end-of-backward callback)"""
    monkeypatch.setattr(ops.GradReducer, "enabled", mode == "acc_on")
    ops.GradReducer.begin_step(torch.device(DEV, torch.cuda.current_device()))
    pg = [p.to(DEV).requires_grad_(True) for p in packed]
    eg = [e.to(DEV) for e in eps]
    if mode == "returned":
        tg, gtheta = theta.to(DEV).requires_grad_(True), None
    else:
        tg, gtheta = theta.to(DEV), torch.ones(theta.shape, device=DEV)
    lat, z = ops.moe_ksample(tg, pg, eg, laplace, gtheta, beta=beta)
    pi = lat.grad_fn.saved_tensors[1].detach().clone()
    ((lat * dlat.to(DEV)).sum() + (z * dz.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    dtheta = tg.grad if mode == "returned" else gtheta - 1.0
    return lat.detach(), z.detach(), [p.grad for p in pg], dtheta, pi


def _moe_cases():
    """every (M, D, family) with K, B, beta and the theta-gradient form rotated so that each value of each meets every
    M and both sides of every slot boundary"""
    Ks, Bs, betas, modes = (1, 3, 30), (1, 5, 127), (1.0, 0.5, 2.0), ("returned", "acc_off", "acc_on")
    out = []
    for j, (M, D) in enumerate(itertools.product((2, 3, 4), (1, 20, 63, 64, 65, 128, 200, 256))):
        for f, fam in enumerate(("normal", "laplace", "mixed")):
            out.append((M, D, fam, Ks[(j + f) % 3], Bs[(j // 3 + 2 * f) % 3], betas[(j + 2 * f) % 3],
                        modes[(j // 2 + f) % 3]))
    return out


@pytest.mark.parametrize("M,D,fam,K,B,beta,mode", _moe_cases())
def test_moe_ksample_fwd_bwd(ops, monkeypatch, M, D, fam, K, B, beta, mode):
    laplace = [fam == "laplace" or (fam == "mixed" and m % 2 == 0) for m in range(M)]
    theta, packed, eps, dlat, dz = _moe_inputs(M, K, B, D, laplace, seed=1000 * M + D)
    t64 = theta.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in packed]
    lr, zr, pir = _ref_moe_ksample(t64, p64, [e.double() for e in eps], laplace, beta)
    ((lr * dlat.double()).sum() + (zr * dz.double()).sum()).backward()
    lat, z, dp, dtheta, pi = _run_moe_ksample(ops, theta, packed, eps, laplace, beta, dlat, dz, mode, monkeypatch)
    check(lat, lr, 1e-5, "lat")
    check(z, zr, 1e-6, "z")
    check(pi, pir, 5e-5, "pi")
    for m in range(M):
        check(dp[m], p64[m].grad, 1e-4, f"dpacked[{m}]")
    check(dtheta, t64.grad, 1e-4, f"dtheta ({mode})")


def test_moe_ksample_laplace_tie_has_zero_subgradient(ops, monkeypatch):
    """eps = 0 on a Laplace coordinate makes z == mu exactly; with the posteriors' means equal there, z == mu_m for every
    m, where torch's |x| has the subgradient 0 -- so must the kernel's sign.  (Posteriors close to each other: pi is not
    one-hot, the other modalities' terms weigh in.)"""
    M, K, B, D = 3, 4, 6, 20
    laplace = [True] * M
    g = torch.Generator().manual_seed(11)
    mu = torch.randn(B, D, generator=g)
    s = 0.8 + 0.2 * torch.rand(B, D, generator=g)
    packed = [torch.cat([mu + 0.05 * torch.randn(B, D, generator=g) * (torch.arange(D) % 3 != 0),
                         s + 0.02 * torch.rand(B, D, generator=g)], -1) for _ in range(M)]
    eps = [_laplace_eps((K, B, D), g) for _ in range(M)]
    for e in eps:
        e[:, :, 0::3] = 0.0      # the coordinates where every mean agrees
    theta = torch.randn(1, D, generator=g) * 0.3
    dlat = torch.randn(M, K, B, generator=g)
    dz = torch.randn(M, K, B, D, generator=g)
    t64 = theta.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in packed]
    lr, zr, pir = _ref_moe_ksample(t64, p64, [e.double() for e in eps], laplace, 1.0)
    ((lr * dlat.double()).sum() + (zr * dz.double()).sum()).backward()
    assert float(pir.detach().max()) < 0.99
    lat, z, dp, dtheta, pi = _run_moe_ksample(ops, theta, packed, eps, laplace, 1.0, dlat, dz, "returned", monkeypatch)
    for m in range(M):
        assert torch.equal(z[m][:, :, 0::3].cpu(), packed[m][:, :D][:, 0::3].expand(K, B, -1)), "z == mu at eps = 0"
    check(lat, lr, 1e-5, "lat")
    for m in range(M):
        check(dp[m], p64[m].grad, 5e-5, f"dpacked[{m}]")
    check(dtheta, t64.grad, 5e-5, "dtheta")


@pytest.mark.parametrize("fam", ["normal", "laplace"])
def test_moe_ksample_far_apart_posteriors_stay_finite(ops, monkeypatch, fam):
    """sum_d log q_m(z) of the M posteriors about 1e3 apart: the log-mean-exp and the weights pi stay finite and exact
    (pi one-hot up to exp(-1e3))"""
    M, K, B, D = 2, 3, 5, 20
    laplace = [fam == "laplace"] * M
    theta, packed, eps, dlat, dz = _moe_inputs(M, K, B, D, laplace, seed=5)
    packed[1][:, :D] += 5.0 if fam == "normal" else 25.0
    packed[0][:, D:] = 0.5
    packed[1][:, D:] = 0.5
    t64 = theta.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in packed]
    lr, zr, pir = _ref_moe_ksample(t64, p64, [e.double() for e in eps], laplace, 1.0)
    lq_gap = float((pir.clamp_min(1e-300).log()[..., 0] - pir.clamp_min(1e-300).log()[..., 1]).abs().min())
    assert lq_gap > 500, lq_gap
    ((lr * dlat.double()).sum() + (zr * dz.double()).sum()).backward()
    lat, z, dp, dtheta, pi = _run_moe_ksample(ops, theta, packed, eps, laplace, 1.0, dlat, dz, "returned", monkeypatch)
    assert bool(torch.isfinite(lat).all()) and bool(torch.isfinite(pi).all())
    check(lat, lr, 1e-5, "lat")
    check(pi, pir, 1e-6, "pi")
    for m in range(M):
        check(dp[m], p64[m].grad, 5e-5, f"dpacked[{m}]")
    check(dtheta, t64.grad, 5e-5, "dtheta")


def test_moe_ksample_rejects_unsupported_shapes(ops, H, hip_lib):
    """D > 256 (four 64-lane slots) and M > 4 are errors, not output"""
    g = torch.Generator().manual_seed(2)
    K, B = 2, 3
    for M, D in ((2, 257), (5, 16)):
        theta, packed, eps, _, _ = _moe_inputs(M, K, B, D, [False] * M, seed=M + D)
        with pytest.raises((RuntimeError, IndexError)):
            ops.moe_ksample(theta.to(DEV), [p.to(DEV) for p in packed], [e.to(DEV) for e in eps], [False] * M)
    # the C ABI itself refuses M = 5 before it reads the argument block (which holds four entries)
    D = 16
    a = H.MoeKArgs()
    keep = []
    for m in range(4):
        p, e, z = torch.randn(B, 2 * D, generator=g).to(DEV), torch.randn(K, B, D, generator=g).to(DEV), \
            torch.empty(K, B, D, device=DEV)
        keep += [p, e, z]
        a.packed[m], a.eps[m], a.z[m], a.laplace[m] = p.data_ptr(), e.data_ptr(), z.data_ptr(), 0
    theta = torch.zeros(1, D, device=DEV)
    lat = torch.full((5 * K * B,), 7.0, device=DEV)
    pi = torch.empty(5 * K * B * 5, device=DEV)
    rc = hip_lib.mmvae_moe_ksample_fwd(ctypes.byref(a), H.ptr(theta), H.ptr(lat), H.ptr(pi), 5, K, B, D, 1.0,
                                       H.stream())
    rc2 = hip_lib.mmvae_moe_ksample_fwd(ctypes.byref(a), H.ptr(theta), H.ptr(lat), H.ptr(pi), 2, K, B, 257, 1.0,
                                        H.stream())
    torch.cuda.synchronize()
    assert rc != 0 and rc2 != 0
    assert bool((lat == 7.0).all()), "a refused call wrote output"


# ---------------------------------------------------------------------------------------------
# DReG and IWAE losses (ops.dreg_loss, ops.iwae_loss) against float64 restatements of the same fp32 inputs
# ---------------------------------------------------------------------------------------------
LAMS = (0.75, 1.5, 0.3125, 2.0)      # distinct per modality, exact in fp32


def _quant(x):
    """multiples of 2^-10: every fp64 partial sum of these is exact, so the logged lpx blocks are order-independent"""
    return torch.round(x * 1024.0) / 1024.0


def _loss_inputs(M, K, B, case, per_sample, seed):
    """lat (M,K,B), rows [own_0, cross_0, ...] (K*B each).  per_sample: IWAE's weights live per (r, k, b), DReG's per
    (r, k) over the batch sum -- an offset meant for lw is spread over the batch for DReG"""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(M, K, B, generator=g) * 2.0 - 5.0
    rows = [_quant(torch.rand(K * B, generator=g) * 4.0) for _ in range(2 * M)]
    sc = 1.0 if per_sample else 1.0 / B
    if case == "onehot":        # one k (IWAE: one (r, k)) above the others by 1e4
        if per_sample:
            lat[0, 0, :] += 1e4
        else:
            lat[:, 0, :] += 1e4 * sc
    elif case == "uniform":     # every lw equal
        lat = lat[0, 0, :].expand(M, K, B).contiguous()
        rows = [torch.zeros(K * B) for _ in range(2 * M)]
    elif case == "tiny":        # every lw about -1e4: exp(lw) underflows without the max subtraction
        lat = lat * 0.01 - 1e4 * sc
    return lat, rows


def _ref_dreg(lat, rows, lam, g):
    """objectives.py:361-387 in float64: lw[r,k] = sum_b lat - lam_r (sum_b own + sum_b cross); loss = -(w lw).mean(0).sum()
    with w = softmax_k lw detached"""
    M, K, B = lat.shape
    l64 = lat.double().requires_grad_(True)
    r64 = [r.double().view(K, B).requires_grad_(True) for r in rows]
    lw = torch.stack([l64[r].sum(-1) - lam[r] * (r64[2 * r].sum(-1) + r64[2 * r + 1].sum(-1)) for r in range(M)])
    with torch.no_grad():
        w = (lw - torch.logsumexp(lw, 1, keepdim=True)).exp()
    loss = -(w * lw).mean(0).sum()
    loss.backward(torch.tensor(g, dtype=F64))
    rec = torch.stack([torch.stack([-lam[r] * r64[2 * r].detach().sum(-1), -lam[r] * r64[2 * r + 1].detach().sum(-1)])
                       for r in range(M)])
    return loss.detach(), rec, l64.grad, [t.grad.reshape(-1) for t in r64]


def _ref_iwae(lat, rows, lam, g):
    """objectives.py:342-359 in float64: lw[r,k,b] = lat - lam_r (own + cross); loss = -sum_b log-mean-exp_{r,k} lw"""
    M, K, B = lat.shape
    l64 = lat.double().requires_grad_(True)
    r64 = [r.double().view(K, B).requires_grad_(True) for r in rows]
    lw = torch.stack([l64[r] - lam[r] * (r64[2 * r] + r64[2 * r + 1]) for r in range(M)])
    loss = -(torch.logsumexp(lw.reshape(M * K, B), 0) - math.log(M * K)).sum()
    loss.backward(torch.tensor(g, dtype=F64))
    rec = torch.stack([torch.stack([-lam[r] * r64[2 * r].detach().reshape(-1), -lam[r] * r64[2 * r + 1].detach().reshape(-1)])
                       for r in range(M)])
    return loss.detach(), rec, l64.grad, [t.grad.reshape(-1) for t in r64]


@pytest.mark.parametrize("kind", ["dreg", "iwae"])
@pytest.mark.parametrize("M,K,B", list(itertools.product((2, 3, 4), (1, 2, 30), (1, 63, 64, 65, 257, 1000))))
def test_dreg_iwae_loss_fwd_bwd(ops, kind, M, K, B):
    lam = LAMS[:M]
    fn, ref = (ops.dreg_loss, _ref_dreg) if kind == "dreg" else (ops.iwae_loss, _ref_iwae)
    gscale = -0.7
    for ci, case in enumerate(("random", "onehot", "uniform", "tiny")):
        lat, rows = _loss_inputs(M, K, B, case, kind == "iwae", seed=100 * M + 10 * K + B + ci)
        lr, recr, dlr, drr = ref(lat, rows, lam, gscale)
        lg = lat.to(DEV).requires_grad_(True)
        rg = [r.to(DEV).requires_grad_(True) for r in rows]
        loss, rec = fn(lg, lam, rg)
        torch.autograd.backward(loss, torch.tensor(gscale, dtype=F64, device=DEV))
        torch.cuda.synchronize()
        what = f"{kind} {case}"
        assert math.isfinite(loss.item()), f"{what}: loss {loss.item()}"
        assert abs(loss.item() - lr.item()) <= 1e-12 * abs(lr.item()) + 1e-300, \
            f"{what}: loss {loss.item()!r} vs {lr.item()!r}"
        assert torch.equal(rec.cpu(), recr), f"{what}: logged lpx blocks differ"
        check_fp32_rounding(lg.grad, dlr, f"{what}: dlat")
        for r in range(M):
            check_fp32_rounding(rg[2 * r].grad, drr[2 * r], f"{what}: d own[{r}]")
            check_fp32_rounding(rg[2 * r + 1].grad, drr[2 * r + 1], f"{what}: d cross[{r}]")


# ---------------------------------------------------------------------------------------------
# ELBO-side helpers (`prior: laplace` elbo, MOE.objective :41-62)
# ---------------------------------------------------------------------------------------------
HELPER_SHAPES = list(itertools.product((1, 63, 64, 65, 200), (1, 7, 130)))


def _packed(B, D, g, lo=0.3, hi=1.5):
    return torch.cat([torch.randn(B, D, generator=g), lo + (hi - lo) * torch.rand(B, D, generator=g)], -1)


@pytest.mark.parametrize("D,B", HELPER_SHAPES)
def test_kl_laplace_normal(ops, D, B):
    """sum_d KL(Laplace(mu, s) || N(0, 1)) (torch.distributions' closed form; utils.py:399-402)"""
    g = torch.Generator().manual_seed(D * 31 + B)
    packed = _packed(B, D, g, 0.1, 2.0)
    gk = torch.randn(B, generator=g)
    p64 = packed.double().requires_grad_(True)
    klr = kl_divergence(Laplace(p64[:, :D], p64[:, D:]), Normal(0.0, 1.0)).sum(-1)
    klr.backward(gk.double())
    pg = packed.to(DEV).requires_grad_(True)
    kl = ops.kl_laplace_normal(pg)
    kl.backward(gk.to(DEV))
    check(kl, klr, 1e-5, "kl")
    check(pg.grad, p64.grad, 1e-6, "dpacked")


@pytest.mark.parametrize("lap", [True, False], ids=["laplace", "normal"])
@pytest.mark.parametrize("D,B", HELPER_SHAPES)
def test_logratio(ops, lap, D, B):
    """lw[b] = sum_d [log q_r(z) - log q_o(z)], gradient into packed_r only (:56-62); every third coordinate has
    z == mu_r exactly (Laplace: the subgradient of |z - mu| there is torch's 0)"""
    g = torch.Generator().manual_seed(D * 17 + B + lap)
    pr, po = _packed(B, D, g), _packed(B, D, g)
    po[:, :D] += 1.0
    z = pr[:, :D] + pr[:, D:] * torch.randn(B, D, generator=g)
    z[:, 0::3] = pr[:, :D][:, 0::3]
    gl = torch.randn(B, generator=g)
    r64 = pr.double().requires_grad_(True)
    o64, z64 = po.double(), z.double()
    lwr = (_dist(lap, r64[:, :D], r64[:, D:]).log_prob(z64) - _dist(lap, o64[:, :D], o64[:, D:]).log_prob(z64)).sum(-1)
    lwr.backward(gl.double())
    rg = pr.to(DEV).requires_grad_(True)
    og = po.to(DEV).requires_grad_(True)
    lw = (ops.laplace_logratio if lap else ops.normal_logratio)(rg, og, z.to(DEV))
    lw.backward(gl.to(DEV))
    check(lw, lwr, 1e-5, "lw")
    check(rg.grad, r64.grad, 1e-6, "dpacked_r")
    assert og.grad is None or not bool(og.grad.any()), "gradient leaked into the detached posterior"
    if lap:
        assert not bool(rg.grad[:, :D][:, 0::3].any()), "d mu at z == mu must be 0"


@pytest.mark.parametrize("n", [1, 63, 65, 257, 1001])
def test_expmul(ops, n):
    g = torch.Generator().manual_seed(n)
    lw = torch.rand(n, generator=g) * 10.0 - 5.0
    r = torch.rand(n, generator=g) * 100.0
    go = torch.randn(n, generator=g)
    l64, r64 = lw.double().requires_grad_(True), r.double().requires_grad_(True)
    outr = l64.exp() * r64
    outr.backward(go.double())
    lg, rg = lw.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    out = ops.expmul(lg, rg)
    out.backward(go.to(DEV))
    check(out, outr, 1e-6, "exp(lw) r")
    check(lg.grad, l64.grad, 1e-6, "dlw")
    check(rg.grad, r64.grad, 1e-6, "dr")


def _grad(t):
    return t.grad if t.grad is not None else torch.zeros_like(t)


@pytest.mark.parametrize("M,B", [(2, 1), (2, 7), (2, 130), (3, 63), (2, 301)])
def test_moe_elbo_drops_zero_rows(ops, M, B):
    """ELBO assembly of the MoE elbo branch (mmvae_models.py:41-77, objectives.py:54-67): rows [own_r, exp(lw) cross_r]
    per modality, one own row of exact zeros and one cross row whose exp(lw < -104) underflows to 0 in fp32.  The
    reference keeps only the rows with lp.sum() != 0: its loss, its row count and every gradient (a dropped row's is 0)"""
    g = torch.Generator().manual_seed(M * 1000 + B)
    own = [torch.rand(B, generator=g) * 50.0 + 1.0 for _ in range(M)]
    own[1] = torch.zeros(B)
    lw = [torch.rand(B, generator=g) * 2.0 - 1.0 for _ in range(M)]
    lw[0] = -105.0 - 20.0 * torch.rand(B, generator=g)
    cross = [torch.rand(B, generator=g) * 50.0 + 1.0 for _ in range(M)]
    kld = torch.rand(M, B, generator=g) * 3.0
    W = [float(x) for x in (0.5, 2.0, 1.0, 0.25, 1.5, 0.75)[:2 * M]]
    beta, gs = 0.7, 1.3
    # the reference's filter, on its own fp32 rows
    rows32 = []
    for r in range(M):
        rows32 += [own[r], torch.exp(lw[r]) * cross[r]]
    keep = [n for n in range(2 * M) if float((rows32[n] * -W[n]).sum()) != 0.0]
    assert len(keep) == 2 * M - 2
    o64 = [t.double().requires_grad_(True) for t in own]
    lw64 = [t.double().requires_grad_(True) for t in lw]
    c64 = [t.double().requires_grad_(True) for t in cross]
    k64 = kld.double().requires_grad_(True)
    rows64 = []
    for r in range(M):
        rows64 += [o64[r], lw64[r].exp() * c64[r]]
    lpx = torch.stack([-W[n] * rows64[n] for n in keep])
    lossr = -(lpx.sum(-1) - beta * k64.sum()).sum() / M
    lossr.backward(torch.tensor(gs, dtype=F64))

    og = [t.to(DEV).requires_grad_(True) for t in own]
    lwg = [t.to(DEV).requires_grad_(True) for t in lw]
    cg = [t.to(DEV).requires_grad_(True) for t in cross]
    kg = kld.to(DEV).requires_grad_(True)
    rows = []
    for r in range(M):
        rows += [og[r], ops.expmul(lwg[r], cg[r])]
    loss = ops.moe_elbo(rows, W, kg, beta, M)
    out = loss.grad_fn.saved_tensors[0]
    loss.backward(torch.tensor(gs, device=DEV))
    torch.cuda.synchronize()
    assert float(out[1]) == len(keep), f"n_nz {float(out[1])} vs {len(keep)}"
    check(loss.reshape(1), lossr.reshape(1), 1e-5, "loss")
    check(kg.grad, k64.grad, 1e-6, "dkld")
    for r in range(M):       # (a row the reference drops never reaches its autograd graph: gradient 0)
        check(og[r].grad, _grad(o64[r]), 1e-6, f"d own[{r}]")
        check(cg[r].grad, _grad(c64[r]), 1e-6, f"d cross[{r}]")
        check(lwg[r].grad, _grad(lw64[r]), 1e-6, f"d lw[{r}]")
    assert not bool(og[1].grad.any()), "the dropped all-zero row got a gradient"


def test_moe_elbo_dropped_row_gets_no_gradient(ops):
    """the op on its own: a row of exact zeros is not in the reference's loss, so its gradient is 0 (not W g / M)"""
    B, M = 9, 2
    g = torch.Generator().manual_seed(3)
    rows = [torch.rand(B, generator=g).to(DEV).requires_grad_(True) for _ in range(2 * M)]
    with torch.no_grad():
        rows[3].zero_()
    kld = torch.rand(M, B, generator=g).to(DEV).requires_grad_(True)
    loss = ops.moe_elbo(rows, [1.0, 1.0, 1.0, 1.0], kld, 1.0, M)
    loss.backward()
    torch.cuda.synchronize()
    for n in range(3):
        assert torch.equal(rows[n].grad.cpu(), torch.full((B,), 0.5))
    assert torch.equal(rows[3].grad.cpu(), torch.zeros(B))
    assert torch.equal(kld.grad.cpu(), torch.full((M, B), 1.5))


# ---------------------------------------------------------------------------------------------
# Device noise (ops.randn, ops.rand_laplace) as distributions; fixed seeds, ~0.1 % critical values
# ---------------------------------------------------------------------------------------------
N_BIG = 1 << 22                  # 4M samples: 8192 / 16384 workgroups wanted, 1024 launched -- the grid-stride loop
N_ODD = 1_000_001


def _ks(x, cdf):
    """Kolmogorov-Smirnov distance of the sample x from the float64 CDF, and its ~0.1 % critical value"""
    x, _ = torch.sort(x.detach().double().cpu().reshape(-1))
    n = x.numel()
    Fx = cdf(x)
    i = torch.arange(1, n + 1, dtype=F64)
    return float(torch.maximum(i / n - Fx, Fx - (i - 1) / n).max()), 1.95 / math.sqrt(n)


def _normal_cdf(x):
    return torch.special.ndtr(x)


def _laplace_cdf(x):
    return torch.where(x < 0, 0.5 * torch.exp(x.clamp_max(0)), 1.0 - 0.5 * torch.exp(-x.clamp_min(0)))


def _corr(a, b):
    a = a.double().cpu().reshape(-1)
    b = b.double().cpu().reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / (a.norm() * b.norm()))


def _state(seed, counter=0):
    return torch.tensor([seed, counter, 0], dtype=torch.int32, device=DEV)


GENS = {"randn": (1.0, _normal_cdf), "rand_laplace": (2.0, _laplace_cdf)}


@pytest.mark.parametrize("n", [N_BIG, N_ODD])
@pytest.mark.parametrize("gen", list(GENS))
def test_noise_distribution(ops, gen, n):
    var, cdf = GENS[gen]
    x = getattr(ops, gen)((n,), _state(20260 + n % 7))
    torch.cuda.synchronize()
    xd = x.double().cpu()
    assert bool(torch.isfinite(xd).all())
    kurt = 3.0 if gen == "randn" else 6.0
    se_mean, se_var = math.sqrt(var / n), var * math.sqrt((kurt - 1.0) / n)
    assert abs(float(xd.mean())) < 5 * se_mean, f"mean {float(xd.mean())}"
    assert abs(float(xd.var()) - var) < 5 * se_var, f"variance {float(xd.var())} vs {var}"
    d, crit = _ks(xd, cdf)
    assert d < crit, f"KS distance {d:.3e} >= {crit:.3e}"
    lim = 5.0 / math.sqrt(n / 2)
    assert abs(_corr(xd[:-1], xd[1:])) < lim, "lag-1 correlation"
    m = n // 2
    assert abs(_corr(xd[0:2 * m:2], xd[1:2 * m:2])) < lim, "even / odd correlation"


def test_randn_box_muller_radius(ops):
    """the pair (x_2i, x_2i+1) of one Box-Muller draw: x_2i^2 + x_2i+1^2 ~ Exp(1/2), and the angle uniform"""
    x = ops.randn((N_BIG,), _state(99)).double().cpu().view(-1, 2)
    r2 = (x * x).sum(-1)
    d, crit = _ks(r2, lambda t: 1.0 - torch.exp(-0.5 * t))
    assert d < crit, f"radius KS distance {d:.3e} >= {crit:.3e}"
    ang = torch.atan2(x[:, 1], x[:, 0])
    d, crit = _ks(ang, lambda t: (t + math.pi) / (2 * math.pi))
    assert d < crit, f"angle KS distance {d:.3e} >= {crit:.3e}"
    assert abs(_corr(r2, ang.abs())) < 5.0 / math.sqrt(r2.numel()), "radius and angle correlated"


@pytest.mark.parametrize("gen", list(GENS))
@pytest.mark.parametrize("n", [1, 7, 1001, N_ODD])
def test_noise_state_advances_once(ops, gen, n):
    """same state -> bit-identical draw; a call moves the counter by exactly one and hands the ticket back to 0"""
    s1, s2 = _state(4242, 17), _state(4242, 17)
    a = getattr(ops, gen)((n,), s1)
    b = getattr(ops, gen)((n,), s2)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert s1.tolist() == [4242, 18, 0] and s2.tolist() == [4242, 18, 0]
    c = getattr(ops, gen)((n,), s1)
    torch.cuda.synchronize()
    assert s1.tolist() == [4242, 19, 0]
    if n > 1:
        assert not torch.equal(a, c), "two consecutive draws repeat"


@pytest.mark.parametrize("gen", list(GENS))
def test_noise_consecutive_and_cross_family_uncorrelated(ops, gen):
    n = N_ODD
    st = _state(31337)
    a = getattr(ops, gen)((n,), st)
    b = getattr(ops, gen)((n,), st)
    other = "rand_laplace" if gen == "randn" else "randn"
    c = getattr(ops, other)((n,), _state(31337))
    torch.cuda.synchronize()
    lim = 5.0 / math.sqrt(n)
    assert abs(_corr(a, b)) < lim, "consecutive draws correlated"
    assert abs(_corr(a, c)) < lim, "randn and rand_laplace from the same state correlated"
    assert abs(_corr(a.abs(), c.abs())) < lim, "|randn| and |rand_laplace| from the same state correlated"


@pytest.mark.parametrize("gen", ["mmvae_randn", "mmvae_rand_laplace"])
@pytest.mark.parametrize("n", [1, 7, 1001, 600_001])
def test_noise_writes_nothing_past_n(H, hip_lib, gen, n):
    """through the C ABI into a slice of a sentinel-filled buffer: exactly the n elements change"""
    pad = 256
    buf = torch.full((pad + n + pad,), 12345.0, device=DEV)
    st = _state(7)
    rc = getattr(hip_lib, gen)(buf[pad:].data_ptr(), n, H.ptr(st), H.stream())
    torch.cuda.synchronize()
    assert rc == 0
    b = buf.cpu()
    assert bool((b[:pad] == 12345.0).all()) and bool((b[pad + n:] == 12345.0).all()), "write outside [0, n)"
    assert bool(torch.isfinite(b[pad:pad + n]).all()) and not bool((b[pad:pad + n] == 12345.0).any())


def test_moe_model_draws_each_family(ops, monkeypatch):
    """the MoE dreg objective without eps_override: each modality's noise from its own family (one Laplace, one Normal
    posterior), checked on what reached ops.moe_ksample"""
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import MS_MODS, config_from_mods, mnist_svhn_batch
    seen = []
    real = ops.moe_ksample

    def spy(theta, packed, eps, laplace, gtheta=None, beta=1.0):
        seen.append(([e.detach().clone() for e in eps], list(laplace)))
        return real(theta, packed, eps, laplace, gtheta, beta)

    monkeypatch.setattr(ops, "moe_ksample", spy)
    K, B, D = 30, 32, 20
    mods = [dict(MS_MODS[0], prior="laplace"), dict(MS_MODS[1], prior="normal")]
    cfg, dims = config_from_mods("moe", mods, D, batch_size=B, obj="dreg", K=K)
    torch.manual_seed(5)
    tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
    tr.model.eps_override = None
    out = tr.model.objective(mnist_svhn_batch(B, seed=2, device=DEV))
    torch.cuda.synchronize()
    assert math.isfinite(out["loss"].item())
    assert len(seen) == 1
    eps, laplace = seen[0]
    assert laplace == [True, False]
    for m, (e, cdf) in enumerate(zip(eps, (_laplace_cdf, _normal_cdf))):
        assert e.shape == (K, B, D)
        d, crit = _ks(e, cdf)
        assert d < crit, f"modality {m}: KS distance {d:.3e} >= {crit:.3e} from its own family"
    assert abs(_corr(eps[0], eps[1])) < 5.0 / math.sqrt(K * B * D)
