"""Timing of the MMVM path on the GPU box (no fallback: needs the MI355X).  Writes profiles/mmvm_timing.txt (--out) and
prints one JSON line.

(a) ops.mixprior_fusion forward + backward (csrc/mixprior.hip: one launch each way + the fold of the prior gradient)
    against the same outputs composed from torch-ROCm float32 ops with autograd (tests/mixprior_reference.py on the device,
    the plain form: the absolute log-densities and their logsumexp, the cheaper one to compose), raw heads off, at B = 128,
    D = 32, E in {2, 3, 5} and B = 1000, D = 64, E = 2.  Both sides eager, issued from Python.
(b) ms/step of the captured step (trainer.capture / fused_step) of mmvm, moe (obj elbo), mmjsd and mopoe on the CdSprites+
    towers at B = 128 (the cfg2 shapes: D = 32, T = 32) and on the image + text + action towers (the cfg5 shapes: Ta = 100),
    one after the other in this process.

Every shape warmed up; a figure is the median over `--windows` windows of `--calls` calls (steps), device events around a
window that ends in a synchronise; the two sides of (a) alternate window by window.  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import mixprior_reference as R
from bench_mvtcae import bench_step, window
from multimodal_vae_comparison_amd import ops

DEV = "cuda"
FUSION_SHAPES = [(128, 32, 2), (128, 32, 3), (128, 32, 5), (1000, 64, 2)]      # (B, D, E)
MIXERS = ("mmvm", "moe", "mmjsd", "mopoe")


def bench_fusion(B, D, E, windows, calls):
    inp = R.make_inputs(R.Case(E, D, B))
    heads = [h.to(DEV).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].to(DEV).requires_grad_(True)
    eps, gkl, gz = inp["eps"].to(DEV), inp["gkl"].to(DEV), inp["gz"].to(DEV)
    gzs = list(gz.unbind(0))
    leaves = [theta] + heads

    def hip():
        z, kl, _ = ops.mixprior_fusion(theta, heads, eps)
        return torch.autograd.grad([kl, *z], leaves, [gkl, *gzs])

    def composed():
        z, kl, _ = R.mixprior_reference(theta, heads, eps, form="plain")
        return torch.autograd.grad([kl, z], leaves, [gkl, gz])

    for _ in range(20):
        a, b = hip(), composed()
    dev = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b))
    ms = {"hip": [], "torch": []}
    for _ in range(windows):
        ms["torch"].append(window(composed, calls))
        ms["hip"].append(window(hip, calls))
    return {"B": B, "D": D, "E": E, "hip_ms": ms["hip"], "torch_ms": ms["torch"], "grad_dev": dev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmvm_timing.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--skip-steps", action="store_true", help="(a) only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mmvm.py needs the MI355X"
    med = statistics.median
    lines = [f"MMVM timing, one MI355X (tools/bench_mmvm.py): fp32, every shape warmed up, median of {args.windows} windows of "
             f"{args.calls} calls, device events around a window that ends in a synchronise", "",
             "(a) ops.mixprior_fusion forward + backward (2 launches + the prior-gradient fold) vs the same outputs composed from",
             "    torch-ROCm float32 ops with autograd (absolute log-densities and their logsumexp: the cheaper form), both eager,",
             "    ms per call (windows alternate composed, HIP):"]

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    fusion, steps = [], []
    for B, D, E in FUSION_SHAPES:
        r = bench_fusion(B, D, E, args.windows, args.calls)
        fusion.append(r)
        h, t = med(r["hip_ms"]), med(r["torch_ms"])
        lines.append(f"    B {B:4d} D {D:2d} E {E}: HIP {h:.4f}  composed {t:.4f}  HIP/composed {h / t:.3f}  (HIP min-max "
                     f"{min(r['hip_ms']):.4f}-{max(r['hip_ms']):.4f}, composed {min(r['torch_ms']):.4f}-{max(r['torch_ms']):.4f}; "
                     f"gradients deviate {r['grad_dev']:.1e} relative)")
        flush()
    if not args.skip_steps:
        n = max(args.calls // 2, 1)
        lines += ["", f"(b) captured training step (objective + backward + Adam in one hipGraph), ms/step, B = 128, D = 32, T = 32, windows of "
                      f"{n} steps, the eight models one after the other:"]
        for towers, what in ((2, "CdSprites+ towers (cfg2 shapes)"), (3, "image + text + actions (cfg5 shapes, Ta = 100)")):
            base = None
            for mixing in MIXERS:
                r = bench_step(mixing, towers, args.windows, n)
                steps.append(r)
                m = med(r["ms"])
                base = m if base is None else base
                lines.append(f"    {what}: {mixing:6s} {m:.3f}  (min-max {min(r['ms']):.3f}-{max(r['ms']):.3f}; "
                             f"{r['abi_calls']} C-ABI calls per step; {mixing}/mmvm {m / base:.2f})")
                flush()
    print("\n".join(lines))
    print(json.dumps({"mixprior_fusion": fusion, "steps": steps}))


if __name__ == "__main__":
    main()
