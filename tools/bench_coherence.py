"""Timing of the generation-coherence evaluation on the GPU box (no fallback: needs the MI355X).  Writes
profiles/coherence_timing.txt (--out) and prints one JSON line.

(a) one evaluation as the reference runs it: cross_coherence over N = 250 test pairs plus joint_coherence at n = 64
    (level 5, five classifiers, MoPoE on the CdSprites+ towers), and the same at N = 10 000; batches of 250.
(b) ops.cls_head (five heads, one launch) against the same heads composed from what the package had before it: per
    classifier a torch.relu, two ops.linear (the second with a ReLU on its input) and torch.argmax, at N = 250 and
    N = 10 000.  Composition and kernel alternated, twice each.
Reported, not gated.  Device events around whole calls that end in a synchronise; every shape warmed up first."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from multimodal_vae_comparison_amd import coherence as coh
from multimodal_vae_comparison_amd import hipops as H
from multimodal_vae_comparison_amd import ops

DEV = "cuda"
LEVEL, T, D = 5, 45, 32


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


def bench_head(N, reps):
    g = torch.Generator().manual_seed(N)
    C = [len(coh.CLASS_NAMES[a]) for a in coh.LEVEL_ATTRIBUTES[LEVEL]]
    A, Cmax = len(C), max(C)
    feats = (torch.randn(A, N, 512, generator=g) - 1.0).to(DEV)
    W1 = ((torch.rand(A, 256, 512, generator=g) * 2 - 1) / 512 ** 0.5).to(DEV)
    b1 = ((torch.rand(A, 256, generator=g) * 2 - 1) / 512 ** 0.5).to(DEV)
    W2 = ((torch.rand(A, Cmax, 256, generator=g) * 2 - 1) / 16).to(DEV)
    b2 = ((torch.rand(A, Cmax, generator=g) * 2 - 1) / 16).to(DEV)
    labels = torch.stack([torch.randint(-1, c, (N,), generator=g) for c in C]).int().to(DEV)
    w2 = [W2[a, :C[a]].contiguous() for a in range(A)]
    bb2 = [b2[a, :C[a]].contiguous() for a in range(A)]

    def kern():
        return ops.cls_head(feats, W1, b1, W2, b2, C, labels=labels)

    def comp():
        n_ok = torch.zeros(N, dtype=torch.int32, device=DEV)
        for a in range(A):
            h = ops.linear(torch.relu(feats[a]), W1[a], b1[a])
            pred = torch.argmax(ops.linear(h, w2[a], bb2[a], H.ACT_RELU), dim=-1)
            n_ok += ((labels[a] >= 0) & (pred == labels[a])).int()
        return n_ok

    with torch.no_grad():
        same = bool(torch.equal(kern()["n_correct"], comp()))
        kern(), comp()
        tk, tc = [], []
        for _ in range(2):
            tc.append(timed(comp, reps))
            tk.append(timed(kern, reps))
    return {"N": N, "kernel_ms": tk, "composed_ms": tc, "ratio": min(tk) / min(tc), "same_counts": same}


def bench_eval(N, reps):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import cdsprites_batch, cdsprites_config
    torch.manual_seed(0)
    tr = MultimodalVAE(cdsprites_config("mopoe", D), device=DEV)
    tr.model.eval()
    cls = coh.AttributeClassifiers.for_level(LEVEL).to(DEV)
    batches = [cdsprites_batch(min(250, N - i), T, seed=3 + i, device=DEV) for i in range(0, N, 250)]

    def run():
        tr.model.cross_coherence(batches, cls, LEVEL)
        tr.model.joint_coherence(cls, LEVEL, n=64)

    run()
    return {"N": N, "eval_ms": [timed(run, reps) for _ in range(2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coherence_timing.txt"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_coherence.py needs the MI355X"
    res = {"head": [bench_head(250, args.reps), bench_head(10000, args.reps)],
           "eval": [bench_eval(250, max(args.reps // 4, 2)), bench_eval(10000, 2)]}
    lines = ["generation coherence, one MI355X (tools/bench_coherence.py)", ""]
    for h in res["head"]:
        lines.append(f"cls_head A 5 N {h['N']:6d}: kernel {min(h['kernel_ms']):.4f} ms  composed {min(h['composed_ms']):.4f} ms"
                     f"  kernel/composed {h['ratio']:.3f}  (runs: kernel {h['kernel_ms']}, composed {h['composed_ms']};"
                     f" same counts: {h['same_counts']})")
    for e in res["eval"]:
        lines.append(f"cross (N {e['N']}) + joint (n 64), level 5, MoPoE D {D} T {T}: {min(e['eval_ms']):.2f} ms"
                     f"  (runs: {e['eval_ms']})")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
