"""What tests/test_tc_fusion_gpu.py measures the total-correlation fusion (csrc/tcfusion.hip: mmvae_tc_fusion_fwd / _bwd,
ops.tc_fusion) against: a float64 restatement of the op in plain torch, differentiable by autograd, the deterministic
inputs of every case, the case tables and the part-by-part comparison.  tests/test_tc_reference_host.py pins the
restatement to torch.distributions on the CPU.

The op: head e is (B, 2 D) = [mu_e | lv_e]; raw: lv_e = softmax(u_e, -1) + 1e-6.  T_e = 1 / (exp(lv_e) + 1e-8),
P = sum_e T_e, mu_J = sum_e mu_e T_e / P, V_J = 1 / P (no prior expert), z = mu_J + V_J eps.  Prior scale sp =
softmax(theta) D.  kl row E = sum_d KL(N(mu_J, sigma = V_J) || N(0, sp)); row e = sum_d KL(N(mu_J, sigma = V_J) ||
N(mu_e, sigma = 1 / T_e)) = sum_d [-log(T_e V_J) + T_e^2 (V_J^2 + (mu_J - mu_e)^2) / 2 - 1 / 2].  Nothing is detached."""
import torch
import torch.nn.functional as F

from poe_reference import MAX_WAVES, TOL_GRAD, TOL_JOINT, TOL_KL, TOL_Z, Parts, rel_err, split_packed  # noqa: F401

F64 = torch.float64


def tc_reference(theta, packed, eps, raw=False):
    """-> joint (2,B,D), kl (E+1,B), z (B,D), in the dtype of the inputs (float64 for the tests' reference)"""
    D = packed[0].shape[1] // 2
    assert theta.shape == (1, D) and eps.shape == (packed[0].shape[0], D)
    sp = F.softmax(theta, dim=1) * D
    mus = [p[:, :D] for p in packed]
    lvs = [(F.softmax(p[:, D:], -1) + 1e-6) if raw else p[:, D:] for p in packed]
    T = [1.0 / (torch.exp(l) + 1e-8) for l in lvs]
    P = sum(T)
    muJ = sum(m * t for m, t in zip(mus, T)) / P
    varJ = 1.0 / P
    rows = [(-(t * varJ).log() + 0.5 * t * t * (varJ * varJ + (muJ - m) ** 2) - 0.5).sum(-1) for m, t in zip(mus, T)]
    vr = (varJ / sp) ** 2
    rows.append((0.5 * (vr + (muJ / sp) ** 2 - 1 - vr.log())).sum(-1))
    return torch.stack([muJ, varJ]), torch.stack(rows), muJ + varJ * eps


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
class Case:
    """one input recipe: everything a test needs is drawn from ONE seeded CPU generator in make_inputs"""

    def __init__(self, E, D, B, raw=False, theta0=False, spike=False):
        self.E, self.D, self.B, self.raw, self.theta0, self.spike = E, D, B, raw, theta0, spike
        self.name = f"E{E}-D{D}-B{B}" + ("-raw" if raw else "") + ("-theta0" if theta0 else "") + ("-spike" if spike else "")

    def __repr__(self):
        return self.name


def _pids(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


B0 = 37          # more than one workgroup (4 rows each), the last one partly idle
WIDTHS = (1, 8, 63, 64, 65, 256)      # one column; inside, one below, at and one above the 64 lanes; every column slot
EXPERTS = (1, 2, 3, 5, 8)
ROWS = (1, 5, 1100)                   # one row; fewer than two workgroups; a wave's second and third row (> 2 MAX_WAVES)

WIDTH_CASES = _pids([Case(2, D, B0, raw=raw) for D in WIDTHS for raw in (False, True)])
EXPERT_CASES = _pids([Case(E, 8, B0, raw=raw) for E in EXPERTS for raw in (False, True)]
                     + [Case(8, 256, 7, raw=raw) for raw in (False, True)])
ROW_CASES = _pids([Case(2, 32, B, raw=raw) for B in ROWS for raw in (False, True)] + [Case(3, 70, 1100, raw=True)])
SPIKE_CASES = _pids([Case(2, 32, B0, raw=True, spike=True), Case(2, 70, B0, raw=True, spike=True)])
THETA0_CASES = _pids([Case(2, 8, B0, theta0=True), Case(3, 70, B0, raw=True, theta0=True)])
ALL_CASES = _pids(WIDTH_CASES + [c for c in EXPERT_CASES if c.name not in {w.name for w in WIDTH_CASES}] + ROW_CASES
                  + SPIKE_CASES + THETA0_CASES)
# one case per width class for the tests of the plumbing around the kernels
FAMILY_CASES = [Case(3, 32, B0), Case(3, 70, B0, raw=True)]
# (116 and 129 rows leave 29 and 33 partial rows: the first counts at which one wave of the fold enters its 8-way unrolled
# loop and another does not)
THETA_CASES = _pids([Case(2, D, B, raw=raw) for D, raw in ((32, True), (70, False)) for B in (5, 116, 129, 1100)])
SINGLE_CASES = _pids([Case(1, D, B0, raw=raw) for D in (8, 70) for raw in (False, True)])


def make_inputs(c):
    """float32 CPU tensors of case c: heads (lv = softmax(randn) + 1e-6; raw: randn), noise, theta, and the upstream
    gradients of kl and z"""
    g = torch.Generator().manual_seed(2000 * c.E + 19 * c.D + c.B + (5 if c.raw else 0))
    heads = []
    for _ in range(c.E):
        mu = torch.randn(c.B, c.D, generator=g)
        u = torch.randn(c.B, c.D, generator=g)
        heads.append(torch.cat([mu, u if c.raw else F.softmax(u, -1) + 1e-6], -1))
    if c.spike:
        # ONE row of expert 0 whose softmax saturates: the other columns' lv is 1e-6 (+ e^-40)
        assert c.raw and c.B > 3 and c.D > 1
        heads[0][3, c.D + c.D // 2] = heads[0][3, c.D:].max() + 40.0
    eps = torch.randn(c.B, c.D, generator=g)
    theta = torch.zeros(1, c.D) if c.theta0 else torch.randn(1, c.D, generator=g) * 0.3
    gkl = torch.randn(c.E + 1, c.B, generator=g)
    gz = torch.randn(c.B, c.D, generator=g)
    return {"heads": heads, "eps": eps, "theta": theta, "gkl": gkl, "gz": gz}


def run_reference(c, inp, dtype=F64, use_kl=True, use_z=True, rows=None):
    """the reference's outputs and gradients for upstream gradients gkl (use_kl; rows: only these KL rows) and gz (use_z)
    -> dict of detached tensors: joint, kl, z, dheads [E x (B, 2 D)], dtheta"""
    heads = [h.detach().clone().to(dtype).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].detach().clone().to(dtype).requires_grad_(True)
    joint, kl, z = tc_reference(theta, heads, inp["eps"].to(dtype), c.raw)
    tot = 0.0
    if use_kl:
        gkl = inp["gkl"].to(dtype)
        if rows is not None:
            keep = torch.zeros(c.E + 1, 1, dtype=dtype)
            keep[list(rows)] = 1
            gkl = gkl * keep
        tot = tot + (kl * gkl).sum()
    if use_z:
        tot = tot + (z * inp["gz"].to(dtype)).sum()
    tot.backward()
    return {"joint": joint.detach(), "kl": kl.detach(), "z": z.detach(),
            "dheads": [h.grad if h.grad is not None else torch.zeros_like(h) for h in heads],
            "dtheta": theta.grad if theta.grad is not None else torch.zeros_like(theta)}


# ---------------------------------------------------------------------------------------------
# part by part
# ---------------------------------------------------------------------------------------------
def check_scaled(parts, part, got, ref, scale, tol, kind=None):
    """max |got - ref| over max |scale|: a part that is analytically 0 (the expert row of ONE expert) is held to the
    maximum of the part it sits beside"""
    got, ref, scale = (t.detach().double().cpu() for t in (got, ref, scale))
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    e = float((got - ref).abs().max()) / max(float(scale.abs().max()), 1e-30)
    parts.rows.append((part, e, tol))
    if parts.worst is not None and kind is not None and e == e:
        parts.worst[kind] = max(parts.worst.get(kind, 0.0), e)
    print(f"{parts.what}: {part}: err {e:.3e} of the scale's maximum (bound {tol:.1e})")


def check_forward(parts, c, joint, kl, z, ref, tol=None):
    """joint mean and variance, z, every KL row on its own float64 maximum; E = 1: the expert row is analytically 0 (the
    joint IS the expert) and is held to 2e-5 of the prior row's maximum.  tol: one bound for every part instead"""
    TOL_JOINT, TOL_Z, TOL_KL = (tol,) * 3 if tol is not None else (globals()[k] for k in ("TOL_JOINT", "TOL_Z", "TOL_KL"))
    parts.check("joint mean", joint[0], ref["joint"][0], TOL_JOINT, "joint")
    parts.check("joint variance", joint[1], ref["joint"][1], TOL_JOINT, "joint")
    parts.check("z", z, ref["z"], TOL_Z, "z")
    assert kl.shape == ref["kl"].shape, f"kl: shape {tuple(kl.shape)} vs {tuple(ref['kl'].shape)}"
    for j in range(c.E + 1):
        if c.E == 1 and j == 0:
            check_scaled(parts, "kl row 0 (one expert: 0)", kl[0], ref["kl"][0], ref["kl"][1], TOL_KL, "kl (one expert)")
        else:
            parts.check(f"kl row {j}", kl[j], ref["kl"][j], TOL_KL, "kl")


def check_backward(parts, c, dheads, dtheta, ref, dtheta_what="dtheta", tol=None):
    """per expert the dmu half and the dlv (raw: du) half, each on its own maximum; dtheta (D = 1: exactly 0)"""
    TOL_GRAD = tol if tol is not None else globals()["TOL_GRAD"]
    for e in range(c.E):
        for half, got, want in zip(("dmu", "du" if c.raw else "dlv"), split_packed(dheads[e], c.D),
                                   split_packed(ref["dheads"][e], c.D)):
            if half == "du" and c.D == 1:
                # the softmax of one logit is the constant 1: the kernel writes 0
                assert not bool(want.any())
                parts.exact_zero(f"du[{e}] (one column: lv = 1 + 1e-6 whatever u is)", got)
            else:
                parts.check(f"{half}[{e}]", got, want, TOL_GRAD, half)
    if dtheta is not None:
        if c.D == 1:
            assert not bool(ref["dtheta"].any())
            parts.exact_zero(f"{dtheta_what} (D = 1: softmax of one element is 1, the fold must give 0.0)", dtheta)
        else:
            parts.check(dtheta_what, dtheta, ref["dtheta"], TOL_GRAD, "dtheta")
