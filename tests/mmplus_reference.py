"""What tests/test_mmplus_fusion_gpu.py measures MMVAE+'s latent op (csrc/mmplus.hip: mmvae_mmplus_fwd / _bwd,
ops.mmplus_fusion) against: a float64 restatement of the op in plain torch, differentiable by autograd, the deterministic
inputs of every case, the case tables and the part-by-part comparison.  tests/test_mmplus_reference_host.py pins the
restatement to torch.distributions on the CPU.

The op: head e is (B, 2 W) = [mu_e | lv_e], W = D + P; raw: lv_e = softmax(u_e, -1) + 1e-6 over all W columns.  Columns
[0, D) are the shared posterior q_e^u = N(mu, sigma = lv), columns [D, W) the private one q_e^w; p(u) = N(0, sp), sp =
softmax(theta) D; p(w) = N(0, 1).  With u_m = mu_m^u + sigma_m^u eps_u[m], w_m = mu_m^w + sigma_m^w eps_w[m]:
    z[n] (E B, W)  row m B + b = [u_m[b] | w_m[b]] if n == m, else [u_m[b] | s eps_a[n][m][b]]
    kl row m       = log q_m^u(u_m) - log (1/E) sum_j q_j^u(u_m)       (mixprior_reference on the shared columns)
    kl row E + m   = sum_d KL(q_m^u || N(0, sp))
    kl row 2E + m  = sum_p KL(q_m^w || N(0, 1))
    resp[m][j]     = q_j^u(u_m) / sum_i q_i^u(u_m)
Nothing is detached.  The reference takes the float32 inputs cast up: the device sees the same numbers.

The shared columns follow mixprior_reference's OVERLAPPING recipe (a common base, scales with spread(D) around one
value), and run_reference keeps its condition: at least half of the (m, b) rows hold their largest responsibility below
0.9 wherever E > 1 and E B >= 20 -- on saturated inputs kl_mix is log E to the last bit and its gradient exactly 0, which
a kernel that computes nothing passes.  The `far` family keeps independent means for the saturated path.  The private
columns have independent means of 0.5 randn and the shared columns' scale recipe (raw: the same logits, so that the one
softmax over W gives both blocks scales around 1 / W)."""
import math

import torch
import torch.nn.functional as F

import mixprior_reference as MR
from mixprior_reference import TOL_RESP, overlap_fraction, spread  # noqa: F401
from poe_reference import TOL_GRAD, TOL_KL, TOL_Z, Parts, rel_err, split_packed  # noqa: F401

F64 = torch.float64


def posteriors(packed, raw):
    """-> ([mu_e (B,W)], [sigma_e (B,W)]) of the heads; raw: one softmax over all W columns"""
    W = packed[0].shape[1] // 2
    return [p[:, :W] for p in packed], [(F.softmax(p[:, W:], -1) + 1e-6) if raw else p[:, W:] for p in packed]


def mmplus_reference(theta, packed, eps_u, eps_w, eps_a, D, aux_scale, raw=False, form="difference"):
    """-> z [E x (E B, W)], kl (3E,B), resp (E,E,B), in the dtype of the inputs.  form: mixprior_reference's"""
    E, (B, W2) = len(packed), packed[0].shape
    W = W2 // 2
    P = W - D
    assert theta.shape == (1, D) and eps_u.shape == (E, B, D) and eps_w.shape == (E, B, P) and eps_a.shape == (E, E, B, P)
    mus, sgs = posteriors(packed, raw)
    shared = [torch.cat([mu[:, :D], sg[:, :D]], -1) for mu, sg in zip(mus, sgs)]
    u, kl_shared, resp = MR.mixprior_reference(theta, shared, eps_u, raw=False, form=form)
    w = [mu[:, D:] + sg[:, D:] * eps_w[m] for m, (mu, sg) in enumerate(zip(mus, sgs))]
    kl_w = [(0.5 * (sg[:, D:] ** 2 + mu[:, D:] ** 2 - 1 - (sg[:, D:] ** 2).log())).sum(-1) for mu, sg in zip(mus, sgs)]
    z = [torch.cat([torch.cat([u[m], w[m] if n == m else aux_scale * eps_a[n, m]], -1) for m in range(E)], 0)
         for n in range(E)]
    return z, torch.cat([kl_shared, torch.stack(kl_w)]), resp


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
class Case:
    """one input recipe: everything a test needs is drawn from ONE seeded CPU generator in make_inputs.  spike: None, or the
    block ("shared" / "private") that holds the column whose logit saturates one row of expert 0's softmax"""

    def __init__(self, E, D, P, B, raw=False, theta0=False, spike=None, far=False, scale=0.5, aux=1.5):
        self.E, self.D, self.P, self.B, self.raw, self.theta0 = E, D, P, B, raw, theta0
        self.spike, self.far, self.scale, self.aux = spike, far, scale, aux
        self.W = D + P
        self.name = (f"E{E}-D{D}+{P}-B{B}" + ("-raw" if raw else "") + ("-theta0" if theta0 else "")
                     + (f"-spike_{spike}" if spike else "") + ("-far" if far else "")
                     + (f"-scale{scale:g}" if scale != 0.5 else "") + (f"-aux{aux:g}" if aux != 1.5 else ""))

    def __repr__(self):
        return self.name

    @property
    def overlaps(self):
        """whether run_reference holds the inputs to the overlap condition (mixprior_reference.Case.overlaps)"""
        return self.E > 1 and not self.far and not self.spike and self.E * self.B >= 20


_pids = MR._pids
B0 = MR.B0       # 37: more than one workgroup (4 rows each), the last one partly idle
# one column each; inside one slot; the private block ending at, starting at and straddling a 64-lane slot; D + P = 256
SPLITS = ((1, 1), (8, 4), (60, 10), (63, 1), (64, 64), (65, 8), (192, 64))
EXPERTS = (1, 2, 3, 5, 8)
ROWS = (1, 5, B0, 1100)               # one row; fewer than two workgroups; several; a wave's second and third row (> 2 x 512)
TINY = 1e-5

WIDTH_CASES = _pids([Case(2, D, P, B0, raw=raw) for D, P in SPLITS for raw in (False, True)])
EXPERT_CASES = _pids([Case(E, 8, 4, B0, raw=raw) for E in EXPERTS for raw in (False, True)]
                     + [Case(8, 192, 64, 7, raw=raw) for raw in (False, True)])
ROW_CASES = _pids([Case(2, 32, 16, B, raw=raw) for B in ROWS for raw in (False, True)] + [Case(3, 60, 10, 1100, raw=True)])
SPIKE_CASES = _pids([Case(2, 32, 16, B0, raw=True, spike="shared"), Case(2, 60, 10, B0, raw=True, spike="private")])
THETA0_CASES = _pids([Case(2, 8, 4, B0, theta0=True), Case(3, 60, 10, B0, raw=True, theta0=True)])
FAR_CASES = _pids([Case(3, 32, 16, B0, far=True), Case(3, 60, 10, B0, raw=True, far=True)])
TINY_CASES = _pids([Case(2, 32, 16, B0, scale=TINY), Case(8, 192, 64, 7, scale=TINY)])
# one case per width class for the tests of the plumbing around the kernels
FAMILY_CASES = [Case(3, 32, 16, B0), Case(3, 60, 10, B0, raw=True)]
# (116 and 129 rows leave 29 and 33 partial rows: the first counts at which one wave of the fold enters its 8-way unrolled
# loop and another does not)
THETA_CASES = _pids([Case(2, D, P, B, raw=raw) for D, P, raw in ((32, 16, True), (60, 10, False)) for B in (5, 116, 129, 1100)])
ALL_CASES = (WIDTH_CASES + EXPERT_CASES + ROW_CASES + SPIKE_CASES + THETA0_CASES + FAR_CASES + TINY_CASES + FAMILY_CASES
             + THETA_CASES)


def make_inputs(c):
    """float32 CPU tensors of case c: heads (B, 2 W), eps_u, eps_w, eps_a, theta, and the upstream gradients of kl (3E,B) and
    of every z[n] (E B, W)"""
    g = torch.Generator().manual_seed(3000 * c.E + 23 * c.D + 301 * c.P + c.B + (5 if c.raw else 0) + (11 if c.far else 0))
    E, B, D, P, W = c.E, c.B, c.D, c.P, c.W
    base = torch.randn(B, D, generator=g)
    w = spread(D)
    heads = []
    for e in range(E):
        U = torch.rand(B, W, generator=g)
        noise = torch.randn(B, D, generator=g)
        if c.raw:
            u = torch.log(1 + w * U) + torch.randn(B, 1, generator=g)
            if c.spike and e == 0:
                # ONE row of expert 0 whose softmax saturates: every other column's sigma is 1e-6 (+ e^-40)
                assert B > 3 and W > 1
                col = D // 2 if c.spike == "shared" else D + P // 2
                u[3, col] = u[3].max() + 40.0
            lv, sg = u, F.softmax(u, -1) + 1e-6
        else:
            assert not c.spike
            lv = sg = c.scale * (1 + w * U)
        mu_u = torch.randn(B, D, generator=g) if c.far else base + sg[:, :D] * noise / math.sqrt(D)
        mu_w = 0.5 * torch.randn(B, P, generator=g)
        heads.append(torch.cat([mu_u, mu_w, lv], -1))
    return {"heads": heads, "eps_u": torch.randn(E, B, D, generator=g), "eps_w": torch.randn(E, B, P, generator=g),
            "eps_a": torch.randn(E, E, B, P, generator=g),
            "theta": torch.zeros(1, D) if c.theta0 else torch.randn(1, D, generator=g) * 0.3,
            "gkl": torch.randn(3 * E, B, generator=g), "gz": torch.randn(E, E * B, W, generator=g)}


def run_reference(c, inp, dtype=F64, use_kl=True, use_z=True, form="difference"):
    """the reference's outputs and gradients for upstream gradients gkl (use_kl) and gz (use_z: True, False, or the decoders n
    whose z[n] has one) -> dict of detached tensors: z [E x (E B, W)], kl, resp, dheads [E x (B, 2 W)], dtheta"""
    heads = [h.detach().clone().to(dtype).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].detach().clone().to(dtype).requires_grad_(True)
    z, kl, resp = mmplus_reference(theta, heads, inp["eps_u"].to(dtype), inp["eps_w"].to(dtype), inp["eps_a"].to(dtype), c.D,
                                   c.aux, c.raw, form)
    if c.overlaps and dtype == F64:
        assert overlap_fraction(resp) >= 0.5, f"{c.name}: only {overlap_fraction(resp):.2f} of the rows overlap"
    with_z = range(c.E) if use_z is True else (() if use_z is False else use_z)
    tot = 0.0
    if use_kl:
        tot = tot + (kl * inp["gkl"].to(dtype)).sum()
    for n in with_z:
        tot = tot + (z[n] * inp["gz"][n].to(dtype)).sum()
    if torch.is_tensor(tot):
        tot.backward()
    return {"z": [t.detach() for t in z], "kl": kl.detach(), "resp": resp.detach(),
            "dheads": [h.grad if h.grad is not None else torch.zeros_like(h) for h in heads],
            "dtheta": theta.grad if theta.grad is not None else torch.zeros_like(theta)}


# ---------------------------------------------------------------------------------------------
# part by part
# ---------------------------------------------------------------------------------------------
def check_forward(parts, c, z, kl, resp, ref):
    """every decoder's batch z[n], the kl_mix, kl_u and kl_w row blocks each on their own float64 maximum; every kl_mix ENTRY
    to TOL_KL max(1, |entry|) absolute; the responsibilities to TOL_RESP absolute; E = 1: kl_mix exactly 0"""
    E = c.E
    assert len(z) == E and tuple(kl.shape) == (3 * E, c.B) and tuple(resp.shape) == (E, E, c.B)
    for n in range(E):
        assert tuple(z[n].shape) == (E * c.B, c.W)
        parts.check(f"z[{n}]", z[n], ref["z"][n], TOL_Z, "z")
    if E == 1:
        assert not bool(ref["kl"][0].any())
        parts.exact_zero("kl_mix (one expert: the mixture IS the expert)", kl[:1])
    else:
        parts.check("kl_mix rows", kl[:E], ref["kl"][:E], TOL_KL, "kl_mix")
    parts.check("kl_u rows", kl[E:2 * E], ref["kl"][E:2 * E], TOL_KL, "kl_u")
    parts.check("kl_w rows", kl[2 * E:], ref["kl"][2 * E:], TOL_KL, "kl_w")
    want = ref["kl"][:E].detach().double().cpu()
    err = float(((kl[:E].detach().double().cpu() - want).abs() / want.abs().clamp(min=1.0)).max())
    MR._absolute(parts, "kl_mix, every entry, over max(1, |entry|)", err, TOL_KL, "kl_mix entry")
    err = float((resp.detach().double().cpu() - ref["resp"].double()).abs().max())
    MR._absolute(parts, "resp", err, TOL_RESP, "resp")


def check_backward(parts, c, dheads, dtheta, ref, dtheta_what="dtheta"):
    """per head the dmu half and the dsigma (raw: du) half over all W columns, each on its own maximum; dtheta (D = 1:
    exactly 0)"""
    for e in range(c.E):
        for half, got, want in zip(("dmu", "du" if c.raw else "dsigma"), split_packed(dheads[e], c.W),
                                   split_packed(ref["dheads"][e], c.W)):
            parts.check(f"{half}[{e}]", got, want, TOL_GRAD, half)
    if dtheta is not None:
        if c.D == 1:
            assert not bool(ref["dtheta"].any())
            parts.exact_zero(f"{dtheta_what} (D = 1: softmax of one element is 1, the fold must give 0.0)", dtheta)
        else:
            parts.check(dtheta_what, dtheta, ref["dtheta"], TOL_GRAD, "dtheta")
