"""Timing of the kernel inception distance's sums on the GPU box (no fallback: needs the MI355X).  Writes
profiles/kid_timing.txt (--out) and prints one JSON line.

N = M = 10 000 rows of seeded relu features (the generator of tests/manifold_reference.py, restated), F = 2048 (pooled
Inception features) and F = 512 (the attribute classifiers' trunk), S = 100 subsets of m = 1000 rows drawn as
ops.kid_draw draws them, the usual kernel (degree 3, gamma 1 / F, coef0 1).  ops.kid_sums -- the index check and both
launches -- against the same sums composed from torch-ROCm float64 ops on the same GPU, never an earlier run of this
code: per subset index_select of the m rows of each set (converted to double), three matmuls, pow, sum, the diagonal
taken out with diagonal().sum(); subset by subset, so that the composition holds 3 m x m doubles at a time.  Both sides
warmed, alternated, three times each; device events around whole calls that end in a synchronise.  Reported with the
largest relative deviation of the 3 S sums; reported, not gated."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from multimodal_vae_comparison_amd import ops

DEV = "cuda"
N = 10000
S, M_SUB, SEED = 100, 1000, 0
DEGREE, COEF0 = 3, 1.0
RUNS = 3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def data(F, seed, shift=0.0, scale=1.0):
    W = np.random.RandomState(7).standard_normal((F, F)) / np.sqrt(F)
    X = (shift + scale * np.random.RandomState(seed).standard_normal((N, F))) @ W + 0.25
    return np.maximum(X, 0.0).astype(np.float32)


def torch_sums(X, Y, idx_x, idx_y, gamma):
    """the composed route: (S, 3) float64, subset by subset"""
    out = torch.empty(idx_x.shape[0], 3, dtype=torch.float64, device=X.device)
    for s in range(idx_x.shape[0]):
        xs, ys = X.index_select(0, idx_x[s]).double(), Y.index_select(0, idx_y[s]).double()
        kxx = torch.pow(gamma * torch.matmul(xs, xs.T) + COEF0, DEGREE)
        kyy = torch.pow(gamma * torch.matmul(ys, ys.T) + COEF0, DEGREE)
        kxy = torch.pow(gamma * torch.matmul(xs, ys.T) + COEF0, DEGREE)
        out[s, 0] = kxx.sum() - kxx.diagonal().sum()
        out[s, 1] = kyy.sum() - kyy.diagonal().sum()
        out[s, 2] = kxy.sum()
    return out


def bench(F):
    X, Y = torch.from_numpy(data(F, 1)).to(DEV), torch.from_numpy(data(F, 2, 0.05, 1.0)).to(DEV)
    idx_x, idx_y = (torch.from_numpy(i).to(DEV) for i in ops.kid_draw(N, N, S, M_SUB, SEED))
    gamma = 1.0 / F
    hip = lambda: ops.kid_sums(X, Y, idx_x, idx_y, degree=DEGREE, gamma=gamma, coef0=COEF0)      # noqa: E731
    composed = lambda: torch_sums(X, Y, idx_x, idx_y, gamma)      # noqa: E731
    for _ in range(2):      # warm-up of every shape both sides use (first calls include code loading)
        hip()
        composed()
    res = {"F": F, "N": N, "S": S, "m": M_SUB, "chunks": ops.H.lib().mmvae_kid_chunks(S, M_SUB), "hip_ms": [], "torch_ms": []}
    for _ in range(RUNS):
        t, out_t = timed(composed)
        res["torch_ms"].append(t)
        t, out_h = timed(hip)
        res["hip_ms"].append(t)
    res["sums_dev"] = float(((out_h - out_t).abs() / out_t.abs()).max())
    m = M_SUB
    mmd2 = out_h[:, 0] / (m * (m - 1)) + out_h[:, 1] / (m * (m - 1)) - 2.0 * out_h[:, 2] / (m * m)
    res["kid"], res["std"] = float(mmd2.mean()), float(mmd2.std(unbiased=False))
    # the arithmetic the sums need: S subsets x (2 half blocks + 1 whole block) of m x m dots of 2 F flops (the symmetric
    # blocks walk the tiles on or above the diagonal: 136 of 256 at m = 1000)
    tiles = (m + 63) // 64
    res["mfma_gflop"] = S * (2 * tiles * (tiles + 1) // 2 + tiles * tiles) * 64 * 64 * 2 * F / 1e9
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kid_timing.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kid.py needs the MI355X"
    res = []
    for F in args.sizes:
        res.append(bench(F))
        print(f"F {F} done", file=sys.stderr, flush=True)
    lines = [f"Kernel inception distance, the sums of S = {S} subsets of m = {M_SUB} rows, one MI355X (tools/bench_kid.py): "
             f"N = M = {N} rows, degree {DEGREE}, gamma 1 / F, coef0 {COEF0:g}, float64, best of {RUNS} warmed, alternated runs; "
             "device events around whole calls.  HIP = ops.kid_sums (the index check, the gathered tile launch, the sum "
             "launch); torch-ROCm composed = per subset index_select, three float64 matmuls, pow, sum", ""]
    for r in res:
        h, t = min(r["hip_ms"]), min(r["torch_ms"])
        lines.append(f"F {r['F']} ({r['chunks']} column chunk(s) per row tile):")
        lines.append(f"  HIP {h:.1f} ms  torch-ROCm composed {t:.1f} ms  HIP/torch {h / t:.2f}  (runs: HIP "
                     f"{[round(x, 1) for x in r['hip_ms']]}, torch {[round(x, 1) for x in r['torch_ms']]})")
        lines.append(f"  {r['mfma_gflop']:.0f} GFLOP of fp64 tile products walked: {r['mfma_gflop'] / h:.1f} TFLOP/s over the "
                     f"whole call; the sums deviate {r['sums_dev']:.1e} relative at the most; kid {r['kid']:.6g} +- {r['std']:.3g}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
