"""Timing of the MVTCAE path on the GPU box (no fallback: needs the MI355X).  Writes profiles/mvtcae_timing.txt (--out) and
prints one JSON line.

(a) ops.tc_fusion forward + backward (csrc/tcfusion.hip: one launch each way + the fold of the prior gradient) against the
    same function composed from torch-ROCm float32 ops with autograd (tests/tc_reference.py on the device), raw heads off,
    at B = 128, D = 32, E in {2, 3, 5} and B = 1000, D = 64, E = 2.  Both sides eager, issued from Python.
(b) ms/step of the captured step (trainer.capture / fused_step) of mvtcae, poe and mopoe on the CdSprites+ towers at B = 128
    (the cfg2 shapes: D = 32, T = 32) and on the image + text + action towers (the cfg5 shapes: Ta = 100), one after the
    other in this process.

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

import tc_reference as R
from multimodal_vae_comparison_amd import ops
from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
from multimodal_vae_comparison_amd.synthetic import CD_MODS, WORKLOADS, cdsprites_batch, config_from_mods, vilanro_batch

DEV = "cuda"
FUSION_SHAPES = [(128, 32, 2), (128, 32, 3), (128, 32, 5), (1000, 64, 2)]      # (B, D, E)


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


def bench_fusion(B, D, E, windows, calls):
    inp = R.make_inputs(R.Case(E, D, B))
    heads = [h.to(DEV).requires_grad_(True) for h in inp["heads"]]
    theta = inp["theta"].to(DEV).requires_grad_(True)
    eps, gkl, gz = inp["eps"].to(DEV), inp["gkl"].to(DEV), inp["gz"].to(DEV)
    leaves = [theta] + heads

    def hip():
        _, kl, z = ops.tc_fusion(theta, heads, eps)
        return torch.autograd.grad([kl, z], leaves, [gkl, gz])

    def composed():
        _, kl, z = R.tc_reference(theta, heads, eps)
        return torch.autograd.grad([kl, z], leaves, [gkl, gz])

    for _ in range(20):
        a, b = hip(), composed()
    dev = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b))
    ms = {"hip": [], "torch": []}
    for _ in range(windows):
        ms["torch"].append(window(composed, calls))
        ms["hip"].append(window(hip, calls))
    return {"B": B, "D": D, "E": E, "hip_ms": ms["hip"], "torch_ms": ms["torch"], "grad_dev": dev}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvtcae_timing.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--skip-steps", action="store_true", help="(a) only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mvtcae.py needs the MI355X"
    med = statistics.median
    lines = [f"MVTCAE timing, one MI355X (tools/bench_mvtcae.py): fp32, every shape warmed up, median of {args.windows} windows of "
             f"{args.calls} calls, device events around a window that ends in a synchronise", "",
             "(a) ops.tc_fusion forward + backward (2 launches + the prior-gradient fold) vs the same function composed from",
             "    torch-ROCm float32 ops with autograd, both eager, ms per call (windows alternate composed, HIP):"]

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
        lines += ["", f"(b) captured training step (objective + backward + Adam in one hipGraph), ms/step, B = 128, D = 32, T = 32, windows of "
                      f"{max(args.calls // 2, 1)} steps, the six models one after the other:"]
        for towers, what in ((2, "CdSprites+ towers (cfg2 shapes)"), (3, "image + text + actions (cfg5 shapes, Ta = 100)")):
            base = None
            for mixing in ("mvtcae", "mopoe", "poe"):
                r = bench_step(mixing, towers, args.windows, max(args.calls // 2, 1))
                steps.append(r)
                m = med(r["ms"])
                base = m if base is None else base
                lines.append(f"    {what}: {mixing:6s} {m:.3f}  (min-max {min(r['ms']):.3f}-{max(r['ms']):.3f}; "
                             f"{r['abi_calls']} C-ABI calls per step; {mixing}/mvtcae {m / base:.2f})")
                flush()
    print("\n".join(lines))
    print(json.dumps({"tc_fusion": fusion, "steps": steps}))


if __name__ == "__main__":
    main()
