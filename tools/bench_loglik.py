"""Timing of the held-out log-likelihood estimator on the GPU box (no fallback: needs the MI355X).

(a) the sampler kernel (ops.mix_ksample_logw) against the torch-op composition of the same definition (the reference of
    tests/test_loglik_gpu.py in fp32 on the device), timed TWICE in the same process, alternating with the kernel: the
    kernel must not be slower than the composition by more than the composition's own run-to-run spread;
(b) a full estimate of cfg2 (MoPoE, B = 128, K = 510: its C = 3 components do not divide 512) against the same estimate assembled from the public ops the
    package had before this estimator (ops.randn, ops.poe_reparam_kl through modality_mixing, torch element-wise
    densities, the decoders, recon_rowsum, torch.logsumexp over the stored (K,B) rows).  Reported, not gated.
Device events around whole calls that end in a synchronise; every shape warmed up first.  Prints one JSON line."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from multimodal_vae_comparison_amd import ops

DEV = "cuda"
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def timed(fn, reps):
    """mean ms per call of `reps` back-to-back calls (device events, synchronised)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def composition(comps, theta, eps):
    """Normal components: z, lw0 with torch ops on the device (fp32)"""
    C, B, D2 = comps.shape
    D = D2 // 2
    K = eps.shape[0]
    sp = F.softmax(theta, -1) * D
    sel = torch.arange(K, device=comps.device) % C
    z = comps[sel][:, :, :D] + comps[sel][:, :, D:] * eps
    lp = (-(z * z) / (2 * sp * sp) - sp.log() - HALF_LOG_2PI).sum(-1)
    lq = torch.stack([(-((z - comps[c, :, :D]) ** 2) / (2 * comps[c, :, D:] ** 2) - comps[c, :, D:].log()
                       - HALF_LOG_2PI).sum(-1) for c in range(C)])
    return z, lp - (torch.logsumexp(lq, 0) - math.log(C))


def bench_sampler(C, K, B, D, reps=200):
    g = torch.Generator().manual_seed(C * 1000 + D)
    comps = torch.stack([torch.cat([torch.randn(B, D, generator=g), 0.5 + torch.rand(B, D, generator=g)], -1)
                         for _ in range(C)]).to(DEV)
    theta = (0.3 * torch.randn(1, D, generator=g)).to(DEV)
    eps = torch.randn(K, B, D, generator=g).to(DEV)
    lap = [False] * C
    kern = lambda: ops.mix_ksample_logw(comps, lap, theta, K, eps=eps)
    comp = lambda: composition(comps, theta, eps)
    zk, lk = kern()
    zc, lc = comp()
    err = float((lk - lc).abs().max() / lc.abs().max())
    for _ in range(10):
        kern()
        comp()
    t = {"comp": [], "kern": []}
    for _ in range(2):      # alternate: composition, kernel, composition, kernel
        t["comp"].append(timed(comp, reps))
        t["kern"].append(timed(kern, reps))
    spread = abs(t["comp"][0] - t["comp"][1])
    return {"C": C, "K": K, "B": B, "D": D, "kernel_ms": t["kern"], "composition_ms": t["comp"],
            "composition_spread_ms": spread, "kernel_vs_composition_max_rel_diff": err,
            "ok": max(t["kern"]) <= min(t["comp"]) + spread}


def composed_estimate(model, batch, K, kc):
    """the estimate of cfg2 from the ops the package had before: same chunking, stored rows, one logsumexp at the end"""
    from multimodal_vae_comparison_amd.models.objectives import recon_rowsum
    names = list(model.vaes.keys())
    with torch.no_grad():
        sub = model.modality_mixing(batch)["subsets"]
        comps = torch.stack([torch.cat([mu[0], var[0]], -1) for mu, var in sub.values()])
        C, B, D2 = comps.shape
        D = D2 // 2
        theta = model._pz_params[1]
        ws = []
        for k0 in range(0, K, kc):
            eps = ops.randn((kc, B, D), model._eval_rng_state)
            z, lw0 = composition(comps, theta, eps)      # (k0 % C == 0: the chunk's components start at 0)
            w = lw0.double()
            for m in names:
                mk = batch[m]["masks"]
                out, _ = model.vaes[m].dec({"latents": z.reshape(1, kc * B, D), "masks": None if mk is None else mk.repeat(kc, 1)})
                w = w - recon_rowsum(model.vaes[m].ltype, out, batch[m]).reshape(kc, B).double()
            ws.append(w)
        return torch.logsumexp(torch.cat(ws), 0) - math.log(K)


def bench_estimate(K=510, reps=5):
    """cfg2: MoPoE, B = 128, C = 3 (K = 510: the multiple of 3 next to the 512 the issue names)"""
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import workload
    torch.manual_seed(0)
    _, cfg, dims, data, _ = workload("cfg2", 128, device=DEV, seed=1)
    tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
    tr.model.eval()
    kc = tr.model.default_k_chunk(K, 3, 128)
    est = lambda: tr.model.estimate_log_likelihood(data, K)
    cmp_ = lambda: composed_estimate(tr.model, data, K, kc)
    a, b = est()["joint"], cmp_()
    for _ in range(2):
        est()
        cmp_()
    t = {"est": [], "comp": []}
    for _ in range(2):
        t["comp"].append(timed(cmp_, reps))
        t["est"].append(timed(est, reps))
    return {"config": "cfg2 mopoe", "B": 128, "K": K, "k_chunk": kc, "estimate_ms": t["est"], "composed_ms": t["comp"],
            "joint_mean": float(a.mean()), "composed_joint_mean": float(b.mean())}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_loglik needs the MI355X"
    res = {"device": torch.cuda.get_device_name(0),
           "sampler": [bench_sampler(*s) for s in ((1, 512, 128, 32), (3, 510, 128, 32), (2, 1000, 64, 20))],
           "estimate": bench_estimate()}
    res["ok"] = all(s["ok"] for s in res["sampler"])
    print(json.dumps(res))
    sys.exit(0 if res["ok"] else 1)
