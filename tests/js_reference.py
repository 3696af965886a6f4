"""What tests/test_js_fusion_gpu.py measures the Jensen-Shannon fusion (csrc/jsfusion.hip: mmvae_js_fusion_fwd / _bwd,
ops.js_fusion) against: a float64 restatement of the op in plain torch, differentiable by autograd, the deterministic
inputs of every case, the case tables and the part-by-part comparison.  tests/test_js_reference_host.py pins the
restatement to torch.distributions on the CPU.

The op: head e is (B, 2 D) = [mu_e | lv_e]; raw: lv_e = softmax(u_e, -1) + 1e-6.  Expert e is N(mu_e, sigma_e = lv_e) (the
head read as the SCALE, as the mixture of experts samples from it), index E is the prior N(0, sp), sp = softmax(theta) D.
With weights pi_0 .. pi_E: T_j = pi_j / sigma_j^2, P = sum_j T_j, f = sum_j T_j mu_j / P: the weighted geometric mean is
N(f, P^-1/2).  kl row j = sum_d KL(N(mu_j, sigma_j) || N(f, P^-1/2)), unweighted; z[b] = mu_s + sigma_s eps[b], s = sel[b]
(no expert with that index: 0).  Nothing is detached.

The case tables and the input recipes are tc_reference's (heads, noise, theta, upstream gradients from one seeded generator
per case); a case's weights and its rows' experts are added here."""
import torch
import torch.nn.functional as F

from poe_reference import MAX_WAVES, TOL_GRAD, TOL_JOINT, TOL_KL, TOL_Z, Parts, rel_err, split_packed  # noqa: F401
from tc_reference import (ALL_CASES, B0, EXPERT_CASES, EXPERTS, FAMILY_CASES, ROW_CASES, ROWS, SPIKE_CASES,  # noqa: F401
                          THETA0_CASES, THETA_CASES, WIDTH_CASES, WIDTHS, Case, check_scaled)
from tc_reference import make_inputs as _tc_inputs

F64 = torch.float64


def js_reference(theta, packed, eps, sel, weights, raw=False, pairwise=True):
    """-> prior (2,B,D) = [f, P^-1/2], kl (E+1,B), z (B,D), in the dtype of the inputs (float64 for the tests' reference).
    pairwise: m_j = mu_j - f formed as sum_i T_i (mu_j - mu_i) / P, the kernel's form (the same number; in float32 it
    is the one that survives an expert whose scale is 1e-6); False: the plain subtraction"""
    E, D = len(packed), packed[0].shape[1] // 2
    assert theta.shape == (1, D) and eps.shape == (packed[0].shape[0], D) and len(weights) == E + 1
    sp = (F.softmax(theta, dim=1) * D).expand_as(eps)
    mus = [p[:, :D] for p in packed] + [torch.zeros_like(eps)]
    sgs = [(F.softmax(p[:, D:], -1) + 1e-6) if raw else p[:, D:] for p in packed] + [sp]
    T = [w / (s * s) for w, s in zip(weights, sgs)]
    P = sum(T)
    f = sum(m * t for m, t in zip(mus, T)) / P
    rows = []
    for mu, s in zip(mus, sgs):
        m = sum(t * (mu - mi) for t, mi in zip(T, mus)) / P if pairwise else mu - f
        rows.append((0.5 * (-(s * s * P).log() + P * (s * s + m * m) - 1)).sum(-1))
    z = sum((sel == e).to(eps.dtype).unsqueeze(1) * (mus[e] + sgs[e] * eps) for e in range(E))
    return torch.stack([f, P.rsqrt()]), torch.stack(rows), z


# ---------------------------------------------------------------------------------------------
# a case's weights and selection
# ---------------------------------------------------------------------------------------------
WEIGHTS = ("uniform", "half", "unequal")
SELECTIONS = ("chunks", "one", "shuffled")


def chunks(B, E):
    """the mixer's rule: sel[b] = (b E) // B, contiguous balanced chunks"""
    return ((torch.arange(B, dtype=torch.int64) * E) // B).to(torch.int32)


def make_weights(E, kind="uniform"):
    """pi_0 .. pi_E, summing to 1.  uniform: 1 / (E + 1) each; half: the prior 0.5, the experts 0.5 / E; unequal: expert e
    in proportion to e + 1, the prior 0.3"""
    if kind == "uniform":
        return [1.0 / (E + 1)] * (E + 1)
    if kind == "half":
        return [0.5 / E] * E + [0.5]
    assert kind == "unequal"
    tot = E * (E + 1) / 2
    return [0.7 * (e + 1) / tot for e in range(E)] + [0.3]


def make_selection(c, kind="chunks"):
    if kind == "chunks":
        return chunks(c.B, c.E)
    if kind == "one":
        return torch.full((c.B,), c.E - 1, dtype=torch.int32)
    assert kind == "shuffled"
    g = torch.Generator().manual_seed(77 + 3 * c.B + c.E)
    return torch.randint(0, c.E, (c.B,), generator=g, dtype=torch.int32)


def make_inputs(c, weights="uniform", sel="chunks"):
    """tc_reference.make_inputs(c) -- float32 CPU heads (lv = softmax(randn) + 1e-6; raw: randn), noise, theta, upstream
    gradients of kl and z -- with the case's weights (E + 1 floats) and its rows' experts (int32 (B,))"""
    inp = _tc_inputs(c)
    inp["weights"] = make_weights(c.E, weights)
    inp["sel"] = make_selection(c, sel)
    return inp


def run_reference(c, inp, dtype=F64, use_kl=True, use_z=True, pairwise=True):
    """the reference's outputs and gradients for upstream gradients gkl (use_kl) and gz (use_z)
    -> dict of detached tensors: prior, kl, z, dheads [E x (B, 2 D)], dtheta"""
    heads = [h.detach().clone().to(dtype).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].detach().clone().to(dtype).requires_grad_(True)
    prior, kl, z = js_reference(theta, heads, inp["eps"].to(dtype), inp["sel"], inp["weights"], c.raw, pairwise)
    tot = 0.0
    if use_kl:
        tot = tot + (kl * inp["gkl"].to(dtype)).sum()
    if use_z:
        tot = tot + (z * inp["gz"].to(dtype)).sum()
    if torch.is_tensor(tot):
        tot.backward()
    return {"prior": prior.detach(), "kl": kl.detach(), "z": z.detach(),
            "dheads": [h.grad if h.grad is not None else torch.zeros_like(h) for h in heads],
            "dtheta": theta.grad if theta.grad is not None else torch.zeros_like(theta)}


# ---------------------------------------------------------------------------------------------
# part by part
# ---------------------------------------------------------------------------------------------
def check_forward(parts, c, prior, kl, z, ref, tol=None):
    """the dynamic prior's mean and scale, z, every KL row on its own float64 maximum; D >= 8: every KL ENTRY on its own
    float64 value as well, always at TOL_KL -- every term of its sum is non-negative, none is near 0.  tol: one bound for
    every part instead"""
    tol_entry = globals()["TOL_KL"]
    TOL_JOINT, TOL_Z, TOL_KL = (tol,) * 3 if tol is not None else (globals()[k] for k in ("TOL_JOINT", "TOL_Z", "TOL_KL"))
    parts.check("prior mean", prior[0], ref["prior"][0], TOL_JOINT, "prior")
    parts.check("prior scale", prior[1], ref["prior"][1], TOL_JOINT, "prior")
    parts.check("z", z, ref["z"], TOL_Z, "z")
    assert kl.shape == ref["kl"].shape, f"kl: shape {tuple(kl.shape)} vs {tuple(ref['kl'].shape)}"
    for j in range(c.E + 1):
        parts.check(f"kl row {j}", kl[j], ref["kl"][j], TOL_KL, "kl")
    if c.D >= 8:
        want = ref["kl"].detach().double().cpu()
        e = float(((kl.detach().double().cpu() - want).abs() / want.abs()).max())
        parts.rows.append(("kl, every entry on its own value", e, tol_entry))
        if parts.worst is not None and e == e:
            parts.worst["kl entry"] = max(parts.worst.get("kl entry", 0.0), e)
        print(f"{parts.what}: kl, every entry on its own value: rel err {e:.3e} (bound {tol_entry:.1e}; smallest entry "
              f"{float(want.abs().min()):.3g})")


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
