"""What tests/test_mixprior_fusion_gpu.py measures the mixture-of-experts prior (csrc/mixprior.hip: mmvae_mixprior_fwd /
_bwd, ops.mixprior_fusion) against: a float64 restatement of the op in plain torch, differentiable by autograd, the
deterministic inputs of every case, the case tables and the part-by-part comparison.  tests/test_mixprior_reference_host.py
pins the restatement to torch.distributions on the CPU.

The op: head e is (B, 2 D) = [mu_e | lv_e]; raw: lv_e = softmax(u_e, -1) + 1e-6.  Expert e is q_e = N(mu_e, sigma_e = lv_e)
(the head read as the SCALE, as the mixture of experts samples from it), the fixed prior N(0, sp), sp = softmax(theta) D.
Every expert gives one sample z_m = mu_m + sigma_m eps_m; h = (1/E) sum_j q_j, densities over the whole D-vector:
    kl row m     = log q_m(z_m) - log h(z_m)            the one-sample estimate of KL(q_m || h)
    kl row E + m = sum_d KL(N(mu_m, sigma_m) || N(0, sp))
    resp[m][j]   = q_j(z_m) / sum_i q_i(z_m)
Nothing is detached.  The reference takes the float32 inputs cast up: the device sees the same numbers.

Inputs OVERLAP: with independent random means every responsibility saturates, kl row m is log E to the last bit and its
gradient exactly 0 -- a backward test on such inputs passes on a kernel that computes nothing.  So mu_e = base + sigma_e
noise / sqrt(D) around a shared base, sigma_e = scale (1 + w U), w = spread(D) (raw heads: u = log(1 + w U) + a row shift,
the same spread around 1 / D), and run_reference asserts that at least half of the (m, b) rows keep their largest responsibility
below 0.9.  The `far` family keeps independent means for the saturated path."""
import math

import torch
import torch.nn.functional as F

from poe_reference import MAX_WAVES, TOL_GRAD, TOL_KL, TOL_Z, Parts, rel_err, split_packed  # noqa: F401

F64 = torch.float64
TOL_RESP = 1e-5      # absolute: a responsibility lies in [0, 1]
FORMS = ("difference", "plain")


def experts(packed, raw):
    """-> ([mu_e], [sigma_e]) of the heads"""
    D = packed[0].shape[1] // 2
    return [p[:, :D] for p in packed], [(F.softmax(p[:, D:], -1) + 1e-6) if raw else p[:, D:] for p in packed]


def mixprior_reference(theta, packed, eps, raw=False, form="difference"):
    """-> z (E,B,D), kl (2E,B), resp (E,E,B), in the dtype of the inputs (float64 for the tests' reference).
    form "difference": log q_j(z_m) - log q_m(z_m) from u_mj = ((mu_m - mu_j) + sigma_m eps_m) / sigma_j, the kernel's
    arithmetic (the same number; in float32 the form that keeps D = 256 and scales of 1e-5); "plain": the absolute
    log-densities, then their logsumexp"""
    assert form in FORMS
    E, (B, D2) = len(packed), packed[0].shape
    D = D2 // 2
    assert theta.shape == (1, D) and eps.shape == (E, B, D)
    sp = F.softmax(theta, dim=1) * D
    mus, sgs = experts(packed, raw)
    z = [mu + sg * eps[m] for m, (mu, sg) in enumerate(zip(mus, sgs))]
    mix, resp = [], []
    for m in range(E):
        if form == "difference":
            cols = []
            for j in range(E):
                if j == m:
                    cols.append(torch.zeros(B, dtype=eps.dtype, device=eps.device))
                    continue
                u = ((mus[m] - mus[j]) + sgs[m] * eps[m]) / sgs[j]
                cols.append((-0.5 * (u - eps[m]) * (u + eps[m]) - (sgs[j] / sgs[m]).log()).sum(-1))
            dl = torch.stack(cols)                                  # (E,B): log q_j(z_m) - log q_m(z_m)
            mix.append(math.log(E) - torch.logsumexp(dl, 0))
        else:
            dl = torch.stack([(-0.5 * ((z[m] - mus[j]) / sgs[j]) ** 2 - sgs[j].log() - 0.5 * math.log(2 * math.pi)).sum(-1)
                              for j in range(E)])                   # (E,B): log q_j(z_m)
            mix.append(dl[m] - (torch.logsumexp(dl, 0) - math.log(E)))
        resp.append(F.softmax(dl, 0))
    std = []
    for mu, sg in zip(mus, sgs):
        vr = (sg / sp) ** 2
        std.append((0.5 * (vr + (mu / sp) ** 2 - 1 - vr.log())).sum(-1))
    return torch.stack(z), torch.stack(mix + std), torch.stack(resp)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
class Case:
    """one input recipe: everything a test needs is drawn from ONE seeded CPU generator in make_inputs"""

    def __init__(self, E, D, B, raw=False, theta0=False, spike=False, far=False, scale=0.5):
        self.E, self.D, self.B, self.raw, self.theta0, self.spike, self.far, self.scale = E, D, B, raw, theta0, spike, far, scale
        self.name = (f"E{E}-D{D}-B{B}" + ("-raw" if raw else "") + ("-theta0" if theta0 else "") + ("-spike" if spike else "")
                     + ("-far" if far else "") + (f"-scale{scale:g}" if scale != 0.5 else ""))

    def __repr__(self):
        return self.name

    @property
    def overlaps(self):
        """whether run_reference holds the inputs to the overlap condition: not the saturated families, and enough
        (m, b) rows for a fraction to mean something (one or five rows decide nothing)"""
        return self.E > 1 and not self.far and not self.spike and self.E * self.B >= 20


def _pids(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


B0 = 37          # more than one workgroup (4 rows each), the last one partly idle
WIDTHS = (1, 8, 63, 64, 65, 256)      # one column; inside, one below, at and one above the 64 lanes; every column slot
EXPERTS = (1, 2, 3, 5, 8)
ROWS = (1, 5, B0, 1100)               # one row; fewer than two workgroups; several; a wave's second and third row (> 2 MAX_WAVES)
TINY = 1e-5

WIDTH_CASES = _pids([Case(2, D, B0, raw=raw) for D in WIDTHS for raw in (False, True)])
EXPERT_CASES = _pids([Case(E, 8, B0, raw=raw) for E in EXPERTS for raw in (False, True)]
                     + [Case(8, 256, 7, raw=raw) for raw in (False, True)])
ROW_CASES = _pids([Case(2, 32, B, raw=raw) for B in ROWS for raw in (False, True)] + [Case(3, 70, 1100, raw=True)])
SPIKE_CASES = _pids([Case(2, 32, B0, raw=True, spike=True), Case(2, 70, B0, raw=True, spike=True)])
THETA0_CASES = _pids([Case(2, 8, B0, theta0=True), Case(3, 70, B0, raw=True, theta0=True)])
FAR_CASES = _pids([Case(3, 32, B0, far=True), Case(3, 70, B0, raw=True, far=True)])
TINY_CASES = _pids([Case(2, 32, B0, scale=TINY), Case(8, 256, 7, scale=TINY)])
# one case per width class for the tests of the plumbing around the kernels
FAMILY_CASES = [Case(3, 32, B0), Case(3, 70, B0, raw=True)]
# (116 and 129 rows leave 29 and 33 partial rows: the first counts at which one wave of the fold enters its 8-way unrolled
# loop and another does not)
THETA_CASES = _pids([Case(2, D, B, raw=raw) for D, raw in ((32, True), (70, False)) for B in (5, 116, 129, 1100)])


def spread(D):
    """the relative spread of the scales: 0.3 up to D = 4, then 0.3 sqrt(4 / D) -- the log-density differences are sums over
    D columns, so a spread that does not shrink with sqrt(D) saturates the wide cases (at 0.3 throughout, D = 256, E = 2: 22 %
    of the rows overlap; D = 8: 58 %)"""
    return 0.3 / math.sqrt(max(D, 4) / 4)


def make_inputs(c):
    """float32 CPU tensors of case c: heads (sigma = scale (1 + spread(D) U); raw: the logits u), noise (E,B,D), theta, and the
    upstream gradients of kl (2E,B) and of every z (E,B,D)"""
    g = torch.Generator().manual_seed(3000 * c.E + 23 * c.D + c.B + (5 if c.raw else 0) + (11 if c.far else 0))
    base = torch.randn(c.B, c.D, generator=g)
    w = spread(c.D)
    heads = []
    for e in range(c.E):
        U = torch.rand(c.B, c.D, generator=g)
        noise = torch.randn(c.B, c.D, generator=g)
        if c.raw:
            u = torch.log(1 + w * U) + torch.randn(c.B, 1, generator=g)
            if c.spike and e == 0:
                # ONE row of expert 0 whose softmax saturates: the other columns' sigma is 1e-6 (+ e^-40)
                assert c.B > 3 and c.D > 1
                u[3, c.D // 2] = u[3].max() + 40.0
            lv, sg = u, F.softmax(u, -1) + 1e-6
        else:
            assert not c.spike
            lv = sg = c.scale * (1 + w * U)
        mu = torch.randn(c.B, c.D, generator=g) if c.far else base + sg * noise / math.sqrt(c.D)
        heads.append(torch.cat([mu, lv], -1))
    eps = torch.randn(c.E, c.B, c.D, generator=g)
    theta = torch.zeros(1, c.D) if c.theta0 else torch.randn(1, c.D, generator=g) * 0.3
    gkl = torch.randn(2 * c.E, c.B, generator=g)
    gz = torch.randn(c.E, c.B, c.D, generator=g)
    return {"heads": heads, "eps": eps, "theta": theta, "gkl": gkl, "gz": gz}


def overlap_fraction(resp):
    """the share of (m, b) rows whose largest responsibility is below 0.9"""
    return float((resp.max(1).values < 0.9).double().mean())


def run_reference(c, inp, dtype=F64, use_kl=True, use_z=True, form="difference"):
    """the reference's outputs and gradients for upstream gradients gkl (use_kl) and gz (use_z: True, False, or the experts
    whose z has one) -> dict of detached tensors: z, kl, resp, dheads [E x (B, 2 D)], dtheta"""
    heads = [h.detach().clone().to(dtype).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].detach().clone().to(dtype).requires_grad_(True)
    z, kl, resp = mixprior_reference(theta, heads, inp["eps"].to(dtype), c.raw, form)
    if c.overlaps and dtype == F64:
        assert overlap_fraction(resp) >= 0.5, f"{c.name}: only {overlap_fraction(resp):.2f} of the rows overlap"
    with_z = range(c.E) if use_z is True else (() if use_z is False else use_z)
    tot = 0.0
    if use_kl:
        tot = tot + (kl * inp["gkl"].to(dtype)).sum()
    for e in with_z:
        tot = tot + (z[e] * inp["gz"][e].to(dtype)).sum()
    if torch.is_tensor(tot):
        tot.backward()
    return {"z": z.detach(), "kl": kl.detach(), "resp": resp.detach(),
            "dheads": [h.grad if h.grad is not None else torch.zeros_like(h) for h in heads],
            "dtheta": theta.grad if theta.grad is not None else torch.zeros_like(theta)}


# ---------------------------------------------------------------------------------------------
# part by part
# ---------------------------------------------------------------------------------------------
def _absolute(parts, part, err, tol, kind):
    parts.rows.append((part, err, tol))
    if parts.worst is not None and math.isfinite(err):
        parts.worst[kind] = max(parts.worst.get(kind, 0.0), err)
    print(f"{parts.what}: {part}: abs err {err:.3e} (bound {tol:.1e})")


def check_forward(parts, c, z, kl, resp, ref, tol=None):
    """every expert's z, the kl_mix rows and the kl_std rows each on their own float64 maximum; every kl_mix ENTRY to
    TOL_KL max(1, |entry|) absolute; the responsibilities to 1e-5 absolute; E = 1: kl_mix exactly 0.  tol: one bound for the
    relative parts instead"""
    tol_entry = globals()["TOL_KL"]
    TOL_Z, TOL_KL = (tol,) * 2 if tol is not None else (globals()[k] for k in ("TOL_Z", "TOL_KL"))
    E = c.E
    assert len(z) == E and tuple(kl.shape) == (2 * E, c.B) and tuple(resp.shape) == (E, E, c.B)
    for e in range(E):
        parts.check(f"z[{e}]", z[e], ref["z"][e], TOL_Z, "z")
    if E == 1:
        assert not bool(ref["kl"][0].any())
        parts.exact_zero("kl_mix (one expert: the mixture IS the expert)", kl[:1])
    else:
        parts.check("kl_mix rows", kl[:E], ref["kl"][:E], TOL_KL, "kl_mix")
    parts.check("kl_std rows", kl[E:], ref["kl"][E:], TOL_KL, "kl_std")
    want = ref["kl"][:E].detach().double().cpu()
    err = float(((kl[:E].detach().double().cpu() - want).abs() / want.abs().clamp(min=1.0)).max())
    _absolute(parts, "kl_mix, every entry, over max(1, |entry|)", err, tol_entry, "kl_mix entry")
    err = float((resp.detach().double().cpu() - ref["resp"].double()).abs().max())
    _absolute(parts, "resp", err, TOL_RESP, "resp")


def check_backward(parts, c, dheads, dtheta, ref, dtheta_what="dtheta", tol=None):
    """per expert the dmu half and the dsigma (raw: du) half, each on its own maximum; dtheta (D = 1: exactly 0)"""
    TOL_GRAD = tol if tol is not None else globals()["TOL_GRAD"]
    for e in range(c.E):
        for half, got, want in zip(("dmu", "du" if c.raw else "dsigma"), split_packed(dheads[e], c.D),
                                   split_packed(ref["dheads"][e], c.D)):
            if half == "du" and c.D == 1:
                # the softmax of one logit is the constant 1: the kernel writes 0
                assert not bool(want.any())
                parts.exact_zero(f"du[{e}] (one column: sigma = 1 + 1e-6 whatever u is)", got)
            else:
                parts.check(f"{half}[{e}]", got, want, TOL_GRAD, half)
    if dtheta is not None:
        if c.D == 1:
            assert not bool(ref["dtheta"].any())
            parts.exact_zero(f"{dtheta_what} (D = 1: softmax of one element is 1, the fold must give 0.0)", dtheta)
        else:
            parts.check(dtheta_what, dtheta, ref["dtheta"], TOL_GRAD, "dtheta")
