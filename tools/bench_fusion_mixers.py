"""Timing of the MVTCAE, mmJSD and MMVM paths and of the MMVAE+ latent op on the GPU box (no fallback: needs the MI355X).  Per mixer (--mixer,
default: the first three, one after the other) it writes profiles/<mixer>_timing.txt (--out-dir) and prints one JSON line.

(a) the mixer's fusion op forward + backward (csrc/tcfusion.hip, jsfusion.hip, mixprior.hip, mmplus.hip: one launch each way
    + the fold of the prior gradient) against the same function composed from torch-ROCm float32 ops with autograd (the
    mixer's tests/*_reference.py on the device, in its cheaper form where it has two), raw heads off, at B = 128, D = 32,
    E in {2, 3, 5} and B = 1000, D = 64, E = 2.  mmJSD: uniform weights, rows in balanced chunks.  MMVAE+: P = D private
    columns, and a third side, the same outputs composed from the library's EXISTING ops (mixprior_fusion on a copy of the
    shared columns, one poe_reparam_kl per private code, the scaled auxiliary draws, rows_fan or torch.cat for the decoder
    batches).  All sides eager, issued from Python.
(b) ms/step of the captured step (trainer.capture / fused_step) of the mixer and of the mixers it is compared with (MIXERS)
    on the CdSprites+ towers at B = 128 (the cfg2 shapes: D = 32, T = 32) and on the image + text + action towers (the cfg5
    shapes: Ta = 100), one after the other in this process.

Every shape warmed up; a figure is the median over `--windows` windows of `--calls` calls (steps), device events around a
window that ends in a synchronise; the two sides of (a) alternate window by window.  Reported, not gated."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

from multimodal_vae_comparison_amd import ops
from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
from multimodal_vae_comparison_amd.synthetic import CD_MODS, WORKLOADS, cdsprites_batch, config_from_mods, vilanro_batch

DEV = "cuda"
FUSION_SHAPES = [(128, 32, 2), (128, 32, 3), (128, 32, 5), (1000, 64, 2)]      # (B, D, E)


# the two sides of (a): t holds theta, heads and the device copies of a reference module's make_inputs -> (outputs,
# their upstream gradients)
def _tc_hip(R, t):
    _, kl, z = ops.tc_fusion(t["theta"], t["heads"], t["eps"])
    return [kl, z], [t["gkl"], t["gz"]]


def _tc_composed(R, t):
    _, kl, z = R.tc_reference(t["theta"], t["heads"], t["eps"])
    return [kl, z], [t["gkl"], t["gz"]]


def _js_hip(R, t):
    _, kl, z = ops.js_fusion(t["theta"], t["heads"], t["eps"], t["sel"], t["weights"])
    return [kl, z], [t["gkl"], t["gz"]]


def _js_composed(R, t):
    _, kl, z = R.js_reference(t["theta"], t["heads"], t["eps"], t["sel"], t["weights"], pairwise=False)
    return [kl, z], [t["gkl"], t["gz"]]


def _mm_hip(R, t):
    z, kl, _ = ops.mixprior_fusion(t["theta"], t["heads"], t["eps"])
    return [kl, *z], [t["gkl"], *t["gz"].unbind(0)]


def _mm_composed(R, t):
    z, kl, _ = R.mixprior_reference(t["theta"], t["heads"], t["eps"], form="plain")
    return [kl, z], [t["gkl"], t["gz"]]


def _plus_hip(R, t):
    z, kl, _ = ops.mmplus_fusion(t["theta"], t["heads"], t["eps_u"], t["eps_w"], t["eps_a"], t["D"], 1.5)
    return [kl, *z], [t["gkl"], *t["gz"].unbind(0)]


def _plus_composed(R, t):
    z, kl, _ = R.mmplus_reference(t["theta"], t["heads"], t["eps_u"], t["eps_w"], t["eps_a"], t["D"], 1.5, form="plain")
    return [kl, *z], [t["gkl"], *t["gz"].unbind(0)]


def _plus_existing(R, t):
    """the latent side of an MMVAE+ step from the ops the library had before mmplus_fusion (heads that are not raw: in a
    step the towers' softmax launches, one per tower and direction, come on top)"""
    heads, D = t["heads"], t["D"]
    E, W = len(heads), heads[0].shape[1] // 2
    P = W - D
    if "theta0" not in t:
        t["theta0"] = torch.zeros(1, P, device=DEV)
        t["gklp"] = [torch.stack([torch.zeros_like(t["gkl"][0]), t["gkl"][2 * E + m]]) for m in range(E)]
    shared = [torch.cat([h[:, :D], h[:, W:W + D]], -1) for h in heads]
    u, kl, _ = ops.mixprior_fusion(t["theta"], shared, t["eps_u"])
    w, klp = [], []
    for m in range(E):
        _, k, z = ops.poe_reparam_kl(t["theta0"], [heads[m]], [t["eps_w"][m]], 2, 0b10, cols=(D, P))
        w.append(z[0])
        klp.append(k)
    aux = 1.5 * t["eps_a"]
    zs = []
    for n in range(E):
        srcs = list(u) + [w[m] if m == n else aux[n, m] for m in range(E)]
        plan = [(E, W, [(m, m, 0) for m in range(E)] + [(E + m, m, D) for m in range(E)])]
        if ops.RowsFan.supported(plan, srcs):
            zs.append(ops.rows_fan(plan, srcs)[0])
        else:
            zs.append(torch.cat([torch.cat(list(u), 0), torch.cat(srcs[E:], 0)], -1))
    return [kl, *klp, *zs], [t["gkl"][:2 * E], *t["gklp"], *t["gz"].unbind(0)]


# mixer -> title, reference module, op, the two sides of (a), what the composed side is, the mixers of (b) (the first: itself)
MIXERS = {
    "mvtcae": dict(title="MVTCAE", ref="tc_reference", op="tc_fusion", hip=_tc_hip, composed=_tc_composed,
                   a=["(a) ops.tc_fusion forward + backward (2 launches + the prior-gradient fold) vs the same function composed from",
                      "    torch-ROCm float32 ops with autograd, both eager, ms per call (windows alternate composed, HIP):"],
                   steps=("mvtcae", "mopoe", "poe")),
    "mmjsd": dict(title="mmJSD", ref="js_reference", op="js_fusion", hip=_js_hip, composed=_js_composed,
                  a=["(a) ops.js_fusion forward + backward (2 launches + the prior-gradient fold) vs the same function composed from",
                     "    torch-ROCm float32 ops with autograd (m_j = mu_j - f: the cheaper form), both eager, ms per call (windows",
                     "    alternate composed, HIP):"],
                  steps=("mmjsd", "moe", "mvtcae", "mopoe")),
    "mmvm": dict(title="MMVM", ref="mixprior_reference", op="mixprior_fusion", hip=_mm_hip, composed=_mm_composed,
                 a=["(a) ops.mixprior_fusion forward + backward (2 launches + the prior-gradient fold) vs the same outputs composed from",
                    "    torch-ROCm float32 ops with autograd (absolute log-densities and their logsumexp: the cheaper form), both eager,",
                    "    ms per call (windows alternate composed, HIP):"],
                 steps=("mmvm", "moe", "mmjsd", "mopoe")),
    "mmvaeplus": dict(title="MMVAE+", ref="mmplus_reference", op="mmplus_fusion", hip=_plus_hip, composed=_plus_composed,
                      existing=_plus_existing, case=lambda R, E, D, B: R.Case(E, D, D, B),
                      a=["(a) ops.mmplus_fusion forward + backward (2 launches + the prior-gradient fold), P = D private columns, vs the",
                         "    same outputs composed from torch-ROCm float32 ops with autograd (absolute log-densities: the cheaper form) and",
                         "    vs their composition from the library's existing ops (mixprior_fusion on a copy of the shared columns, E",
                         "    poe_reparam_kl calls, the scaled auxiliary draws, rows_fan / cat per decoder; heads not raw: the 2 E softmax",
                         "    launches of a step are not in it), all eager, ms per call (windows alternate composed, existing, HIP):"],
                      steps=()),      # (the latent op alone: no mixer is built on it yet)
}


def window(fn, calls):
    """ms per call of `calls` calls of fn"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def bench_fusion(spec, B, D, E, windows, calls):
    R = importlib.import_module(spec["ref"])
    case = spec["case"](R, E, D, B) if "case" in spec else R.Case(E, D, B)
    t = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in R.make_inputs(case).items()}
    t["D"] = D
    t["heads"] = [h.to(DEV).requires_grad_(True) for h in t["heads"]]
    t["theta"].requires_grad_(True)
    leaves = [t["theta"]] + t["heads"]

    def side(f):
        def run():
            outs, gouts = f(R, t)
            return torch.autograd.grad(outs, leaves, gouts)
        return run
    hip, composed = side(spec["hip"]), side(spec["composed"])
    existing = side(spec["existing"]) if "existing" in spec else None
    for _ in range(20):
        a, b = hip(), composed()
        c = existing() if existing else None
    dev = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b))
    ms = {"hip": [], "torch": [], "existing": []}
    for _ in range(windows):
        ms["torch"].append(window(composed, calls))
        if existing:
            ms["existing"].append(window(existing, calls))
        ms["hip"].append(window(hip, calls))
    out = {"B": B, "D": D, "E": E, "hip_ms": ms["hip"], "torch_ms": ms["torch"], "grad_dev": dev}
    if existing:
        out["existing_ms"] = ms["existing"]
        out["existing_grad_dev"] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(c, b))
    return out


def bench_step(mixing, towers, windows, calls):
    if towers == 2:
        mods, batch = CD_MODS, cdsprites_batch(128, 32, seed=1)
    else:
        mods = WORKLOADS["cfg5"][2]
        batch = vilanro_batch(128, 32, mods[2]["data_dim"][0], seed=1)
    cfg, dims = config_from_mods(mixing, mods, 32, batch_size=128)
    torch.manual_seed(0)
    tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
    tr.model.train()
    tr.configure_optimizers()
    batch = {k: {kk: (vv.to(DEV) if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in batch.items()}
    tr.capture(batch, world_size=1)
    for _ in range(20):
        tr.fused_step()
    ms = [window(tr.fused_step, calls) for _ in range(windows)]
    loss = float(tr._static_out["loss"].detach())
    assert loss == loss, f"{mixing}: the captured step's loss is NaN"
    return {"mixing": mixing, "towers": towers, "ms": ms, "abi_calls": int(tr.abi_calls_in_graph), "loss": loss}


def bench_mixer(name, args):
    spec, med = MIXERS[name], statistics.median
    out = os.path.join(args.out_dir, f"{name}_timing.txt")
    lines = [f"{spec['title']} timing, one MI355X (tools/bench_fusion_mixers.py --mixer {name}): fp32, every shape warmed up, "
             f"median of {args.windows} windows of {args.calls} calls, device events around a window that ends in a synchronise",
             ""] + spec["a"]

    def flush():
        os.makedirs(args.out_dir, exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    fusion, steps = [], []
    for B, D, E in FUSION_SHAPES:
        r = bench_fusion(spec, B, D, E, args.windows, args.calls)
        fusion.append(r)
        h, t = med(r["hip_ms"]), med(r["torch_ms"])
        lines.append(f"    B {B:4d} D {D:2d} E {E}: HIP {h:.4f}  composed {t:.4f}  HIP/composed {h / t:.3f}  (HIP min-max "
                     f"{min(r['hip_ms']):.4f}-{max(r['hip_ms']):.4f}, composed {min(r['torch_ms']):.4f}-{max(r['torch_ms']):.4f}; "
                     f"gradients deviate {r['grad_dev']:.1e} relative)")
        if "existing_ms" in r:
            x = med(r["existing_ms"])
            lines.append(f"                     existing ops {x:.4f}  HIP/existing {h / x:.3f}  (min-max {min(r['existing_ms']):.4f}-"
                         f"{max(r['existing_ms']):.4f}; gradients deviate {r['existing_grad_dev']:.1e} relative)")
        flush()
    if not args.skip_steps and spec["steps"]:
        n = max(args.calls // 2, 1)
        lines += ["", f"(b) captured training step (objective + backward + Adam in one hipGraph), ms/step, B = 128, D = 32, T = 32, "
                      f"windows of {n} steps, the {2 * len(spec['steps'])} models one after the other:"]
        for towers, what in ((2, "CdSprites+ towers (cfg2 shapes)"), (3, "image + text + actions (cfg5 shapes, Ta = 100)")):
            base = None
            for mixing in spec["steps"]:
                r = bench_step(mixing, towers, args.windows, n)
                steps.append(r)
                m = med(r["ms"])
                base = m if base is None else base
                lines.append(f"    {what}: {mixing:6s} {m:.3f}  (min-max {min(r['ms']):.3f}-{max(r['ms']):.3f}; "
                             f"{r['abi_calls']} C-ABI calls per step; {mixing}/{name} {m / base:.2f})")
                flush()
    print("\n".join(lines))
    print(json.dumps({"mixer": name, spec["op"]: fusion, "steps": steps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixer", choices=sorted(MIXERS), action="append", help="default: mvtcae, mmjsd and mmvm")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--skip-steps", action="store_true", help="(a) only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fusion_mixers.py needs the MI355X"
    for name in args.mixer or ("mvtcae", "mmjsd", "mmvm"):
        bench_mixer(name, args)


if __name__ == "__main__":
    main()
