"""What tests/test_poe_fusion_gpu.py measures the product-of-experts fusion (csrc/latent.hip: mmvae_poe_reparam_kl_fwd /
_bwd / _bwd_acc, ops.poe_reparam_kl) against: a float64 restatement of the op in plain torch, differentiable by autograd,
the deterministic inputs of every case, the case tables, and the part-by-part comparison.  tests/
test_poe_reference_host.py pins the restatement to torch.distributions and to the closed-form product of Gaussians on the CPU.

The op (models/mmvae_models.py:274-276, utils.py: poe): head e is (B, 2 Dtot) = [mu_e | lv_e]; the experts are columns
[col0, col0 + D) of both halves.  raw: lv_e = softmax(u_e, -1) + 1e-6 over the FULL head width.  T_e = 1 / (exp(lv_e) +
1e-8), P = sum T_e (+ 1 / (1 + 1e-8) with the N(0, 1) prior expert), muJ = sum mu_e T_e / P, varJ = 1 / P;
with_prior == 2: muJ, varJ = mu_0, lv_0 (no product).  Prior scale sp = softmax(theta) D.  KL row j = sum_d KL(N(mu_j,
s_j) || N(0, sp)) with s_e = lv_e and s_E = varJ (the reference uses both as SCALES), rows outside kl_mask are 0.
z_i = muJ + varJ eps_i."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
# of each part's own float64 maximum (the numbers test_hip_ops.test_poe_reparam_kl always used, now per part)
TOL_JOINT, TOL_Z, TOL_KL, TOL_GRAD = 1e-5, 1e-5, 2e-5, 5e-5
MAX_WAVES = 512           # POE_MAX_WAVES: one wave per row up to here, then a wave takes rows wave, wave + 512, ...


def poe_reference(theta, packed, eps, with_prior, kl_mask, cols=None, raw=False):
    """-> joint (2,B,D), kl (E+1,B), z (n_z,B,D), in the dtype of the inputs (float64 for the tests' reference)"""
    with_prior = int(with_prior)
    assert with_prior in (0, 1, 2) and (with_prior != 2 or len(packed) == 1)
    E = len(packed)
    Dtot = packed[0].shape[1] // 2
    col0, D = cols if cols is not None else (0, Dtot)
    assert theta.shape == (1, D)
    sp = F.softmax(theta, dim=1) * D
    mus, lvs = [], []
    for p in packed:
        lv_full = (F.softmax(p[:, Dtot:], -1) + 1e-6) if raw else p[:, Dtot:]
        mus.append(p[:, col0:col0 + D])
        lvs.append(lv_full[:, col0:col0 + D])
    if with_prior == 2:
        muJ, varJ = mus[0], lvs[0]
    else:
        T = [1.0 / (torch.exp(l) + 1e-8) for l in lvs]
        P = sum(T) + (1.0 / (1.0 + 1e-8) if with_prior else 0.0)
        muJ = sum(m * t for m, t in zip(mus, T)) / P
        varJ = 1.0 / P

    def kl(mu, s):
        vr = (s / sp) ** 2
        return (0.5 * (vr + (mu / sp) ** 2 - 1 - vr.log())).sum(-1)

    zero = torch.zeros(muJ.shape[0], dtype=muJ.dtype)
    rows = [kl(m, l) if kl_mask >> e & 1 else zero for e, (m, l) in enumerate(zip(mus, lvs))]
    rows.append(kl(muJ, varJ) if kl_mask >> E & 1 else zero)
    z = torch.stack([muJ + varJ * e for e in eps]) if len(eps) else torch.zeros(0, *muJ.shape, dtype=muJ.dtype)
    return torch.stack([muJ, varJ]), torch.stack(rows), z


def split_packed(g, Dtot):
    """a packed (B, 2 Dtot) tensor (a head output or its gradient) -> its mu half and its lv / raw-logit half"""
    assert g.shape[1] == 2 * Dtot
    return g[:, :Dtot], g[:, Dtot:]


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
class Case:
    """one input recipe: everything a test needs is drawn from ONE seeded CPU generator in make_inputs"""

    def __init__(self, name, E, n_z, D, B, with_prior, kl_mask, raw=False, cols=None, Dtot=None, theta0=False, spike=False):
        self.name, self.E, self.n_z, self.D, self.B = name, E, n_z, D, B
        self.with_prior, self.kl_mask, self.raw, self.cols = with_prior, kl_mask, raw, cols
        self.Dtot = Dtot if Dtot is not None else D
        self.theta0, self.spike = theta0, spike
        assert cols is None or (cols[1] == D and cols[0] + D <= self.Dtot and not raw)
        assert kl_mask < (1 << (E + 1))

    @property
    def fast(self):
        """which kernel family serves it (poe_fast_visit)"""
        return self.D <= 64 and 1 <= self.E <= 3 and self.n_z <= 3

    def __repr__(self):
        return self.name


def _case(E, n_z, D, B, wp=1, mask=None, **kw):
    mask = (1 << (E + 1)) - 1 if mask is None else mask
    name = f"E{E}-nz{n_z}-D{D}-B{B}-wp{wp}-m{mask:b}"
    if kw.get("raw"):
        name += "-raw"
    if kw.get("cols"):
        name += f"-cols{kw['cols'][0]}+{kw['cols'][1]}of{kw['Dtot']}"
    if kw.get("theta0"):
        name += "-theta0"
    if kw.get("spike"):
        name += "-spike"
    return Case(name, E, n_z, D, B, wp, mask, **kw)


def masks(E):
    """nothing (needs n_z > 0), only expert 0, only the joint, the experts without the joint, all"""
    return [0, 1, 1 << E, (1 << E) - 1, (1 << (E + 1)) - 1]


def _pids(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


B0 = 37          # more than one workgroup (4 rows each), the last one partly idle

FAST_CASES = _pids(
    [_case(2, 1, D, B0) for D in (1, 20, 63, 64)]
    + [_case(E, n_z, 32, B0) for E, n_z in ((1, 0), (1, 3), (3, 0), (3, 3))]
    + [_case(2, 2, 32, B) for B in (1, 5, 513, 1100)]
    + [_case(3, 2, 32, B0, mask=m) for m in masks(3)]
    + [_case(2, 1, 32, B0, wp=0)])            # (with_prior = 1: every other line)

GENERIC_CASES = _pids(
    [_case(2, 1, D, B0) for D in (65, 128, 129, 192, 256)]
    + [_case(4, 1, 32, B0), _case(8, 1, 16, B0), _case(2, 4, 32, B0), _case(1, 8, 8, B0)]
    + [_case(8, 8, 256, 7)]
    + [_case(2, 1, 70, B) for B in (513, 1100)]
    + [_case(3, 2, 70, B0, mask=m) for m in masks(3)]
    + [_case(2, 1, 70, B0, wp=0)])

RAW_CASES = _pids(
    [_case(2, 1, D, B0, raw=True) for D in (1, 20, 64, 65, 129, 256)]
    + [_case(4, 1, 1, B0, raw=True)]          # (D = 1 in the generic kernels: du is exactly 0)
    + [_case(2, 2, 32, B, raw=True) for B in (513, 1100)]
    + [_case(2, 1, 70, B, raw=True) for B in (513, 1100)]
    + [_case(1, 3, 32, B0, raw=True), _case(3, 3, 32, B0, raw=True), _case(4, 1, 32, B0, raw=True),
       _case(8, 8, 256, 7, raw=True)]
    + [_case(3, 2, 32, B0, mask=m, raw=True) for m in masks(3)]
    + [_case(3, 2, 70, B0, mask=m, raw=True) for m in masks(3)]
    + [_case(2, 1, 32, B0, wp=0, raw=True), _case(2, 1, 70, B0, wp=0, raw=True)]
    + [_case(2, 2, 32, B0, raw=True, spike=True), _case(2, 2, 70, B0, raw=True, spike=True)])

PASS_THROUGH_CASES = _pids(
    [_case(1, n_z, D, B0, wp=2, mask=m) for D in (20, 70) for n_z in (1, 3) for m in (0, 0b10)]
    + [_case(1, 4, 20, B0, wp=2, mask=m) for m in (0, 0b10)]
    + [_case(1, 1, D, B, wp=2, mask=0b10, theta0=True) for D, B in ((20, B0), (70, B0), (20, 1100))])

# (col0, D) of Dtot; E, with_prior, kl_mask as DMVAE's joint / shared-private calls make them
COLUMN_CASES = _pids(
    [_case(2, 1, D, B0, wp=0, mask=0b100, cols=(c0, D), Dtot=Dtot)
     for Dtot, c0, D in ((30, 0, 20), (30, 20, 10), (150, 0, 70), (150, 70, 80))]
    + [_case(1, 2, D, B0, wp=2, mask=0b10, cols=(c0, D), Dtot=Dtot)
       for Dtot, c0, D in ((30, 0, 20), (30, 20, 10), (150, 0, 70), (150, 70, 80))])

# one case per kernel family for the tests of the plumbing around the kernels
FAMILY_CASES = [_case(3, 3, 32, B0), _case(3, 3, 70, B0)]
THETA_CASES = _pids([_case(2, 1, D, B) for D in (32, 70) for B in (5, 1100)])
NOISE_CASES = [(1, 2, 70, 33), (4, 1, 32, 7)]          # (n_z, E, D, B): the generic kernels' own noise


def make_inputs(c):
    """float32 CPU tensors of case c: heads (lv = softmax(randn) + 1e-6; raw: randn; with_prior 2: |randn| 0.5 + 0.1
    scales), noise, theta, and the upstream gradients of kl and z"""
    g = torch.Generator().manual_seed(1000 * c.E + 17 * c.D + c.B + 7 * c.n_z + (3 if c.raw else 0))
    heads = []
    for _ in range(c.E):
        mu = torch.randn(c.B, c.Dtot, generator=g)
        u = torch.randn(c.B, c.Dtot, generator=g)
        if c.raw:
            lv = u
        elif c.with_prior == 2:
            lv = u.abs() * 0.5 + 0.1
        else:
            lv = F.softmax(u, -1) + 1e-6
        heads.append(torch.cat([mu, lv], -1))
    if c.spike:
        # ONE row of expert 0 whose softmax saturates: the other columns' lv is 1e-6 (+ e^-40), 1 / lv = 1e6
        assert c.raw and c.B > 3 and c.D > 1
        heads[0][3, c.Dtot + c.D // 2] = heads[0][3, c.Dtot:].max() + 40.0
    eps = [torch.randn(c.B, c.D, generator=g) for _ in range(c.n_z)]
    theta = torch.zeros(1, c.D) if c.theta0 else torch.randn(1, c.D, generator=g) * 0.3
    gkl = torch.randn(c.E + 1, c.B, generator=g)
    gz = torch.randn(c.n_z, c.B, c.D, generator=g)
    return {"heads": heads, "eps": eps, "theta": theta, "gkl": gkl, "gz": gz}


def run_reference(c, inp, dtype=F64, use_kl=True, use_z=None):
    """the reference's outputs and gradients for upstream gradients gkl (use_kl) and gz[i] (i in use_z; default: all) ->
    dict of detached tensors: joint, kl, z, dheads [E x (B, 2 Dtot)], dtheta (None where nothing reaches a leaf)"""
    use_z = range(c.n_z) if use_z is None else use_z
    heads = [h.detach().clone().to(dtype).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].detach().clone().to(dtype).requires_grad_(True)
    joint, kl, z = poe_reference(theta, heads, [e.to(dtype) for e in inp["eps"]], c.with_prior, c.kl_mask, c.cols, c.raw)
    tot = 0.0
    if use_kl and c.kl_mask:
        tot = tot + (kl * inp["gkl"].to(dtype)).sum()
    for i in use_z:
        tot = tot + (z[i] * inp["gz"][i].to(dtype)).sum()
    out = {"joint": joint.detach(), "kl": kl.detach(), "z": z.detach(), "dheads": None, "dtheta": None}
    if torch.is_tensor(tot) and tot.requires_grad:
        tot.backward()
        out["dheads"] = [h.grad if h.grad is not None else torch.zeros_like(h) for h in heads]
        out["dtheta"] = theta.grad if theta.grad is not None else torch.zeros_like(theta)
    return out


# ---------------------------------------------------------------------------------------------
# part by part
# ---------------------------------------------------------------------------------------------
def rel_err(a, b):
    """max |a - b| over max |b| (b: the float64 reference); both zero -> 0"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, f"shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if a.numel() == 0:
        return 0.0
    d = float((a - b).abs().max())
    return d / max(float(b.abs().max()), 1e-30) if d != 0.0 else 0.0


class Parts:
    """collects (part, error, bound) of one comparison and asserts them together, naming every part that failed;
    `worst` (a dict shared by a test module) keeps each part's worst error over the suite"""

    def __init__(self, what, worst=None):
        self.what, self.rows, self.worst = what, [], worst

    def check(self, part, got, ref, tol, kind=None):
        e = rel_err(got, ref)
        self.rows.append((part, e, tol))
        if self.worst is not None and kind is not None and math.isfinite(e):
            self.worst[kind] = max(self.worst.get(kind, 0.0), e)
        print(f"{self.what}: {part}: rel err {e:.3e} (bound {tol:.1e})")

    def exact_zero(self, part, got):
        n = int((got.detach() != 0).sum())      # (NaN != 0 counts)
        self.rows.append((part + f" [{n} elements not exactly 0]", 0.0 if n == 0 else float("inf"), 0.0))

    def done(self):
        bad = [f"{p}: {e:.3e} > {t:.1e}" for p, e, t in self.rows if not (math.isfinite(e) and e <= t)]
        assert not bad, f"{self.what}: " + "; ".join(bad)


def check_forward(parts, c, joint, kl, z, ref):
    """joint mean and variance, every KL row of the mask on its own maximum, every other row exactly 0, every z_i"""
    parts.check("joint mean", joint[0], ref["joint"][0], TOL_JOINT, "joint")
    parts.check("joint variance", joint[1], ref["joint"][1], TOL_JOINT, "joint")
    assert kl.shape == ref["kl"].shape, f"kl: shape {tuple(kl.shape)} vs {tuple(ref['kl'].shape)}"
    for j in range(c.E + 1):
        if c.kl_mask >> j & 1:
            parts.check(f"kl row {j}", kl[j], ref["kl"][j], TOL_KL, "kl")
        else:
            parts.exact_zero(f"kl row {j} (outside the mask)", kl[j])
    assert len(z) == c.n_z
    for i in range(c.n_z):
        parts.check(f"z[{i}]", z[i], ref["z"][i], TOL_Z, "z")


def check_backward(parts, c, dheads, dtheta, ref, dtheta_what="dtheta"):
    """per expert the dmu half and the dlv (raw: du) half, each on its own maximum; columns outside `cols` exactly 0;
    dtheta (D = 1: exactly 0)"""
    col0, D = c.cols if c.cols is not None else (0, c.Dtot)
    keep = torch.zeros(c.Dtot, dtype=torch.bool)
    keep[col0:col0 + D] = True
    for e in range(c.E):
        for half, got, want in zip(("dmu", "du" if c.raw else "dlv"), split_packed(dheads[e], c.Dtot),
                                   split_packed(ref["dheads"][e], c.Dtot)):
            if half == "du" and c.Dtot == 1:
                # the softmax of one logit is the constant 1: s (dlv - s dlv) is 0.0 in float32 as in float64
                assert not bool(want.any())
                parts.exact_zero(f"du[{e}] (one column: lv = 1 + 1e-6 whatever u is)", got)
            else:
                parts.check(f"{half}[{e}]", got[:, keep], want[:, keep], TOL_GRAD, half)
            if c.cols is not None:
                assert not bool(want[:, ~keep].any())
                parts.exact_zero(f"{half}[{e}] outside columns [{col0}, {col0 + D})", got[:, ~keep])
    if dtheta is not None:
        if c.D == 1:
            # softmax of one element is exactly 1 and the fold's dot product IS its one term: D s (dsp - dot) = 0
            assert not bool(ref["dtheta"].any())
            parts.exact_zero(f"{dtheta_what} (D = 1: softmax of one element is 1, dot == dsp, so the fold must give 0.0)",
                             dtheta)
        else:
            parts.check(dtheta_what, dtheta, ref["dtheta"], TOL_GRAD, "dtheta")
