"""Timing of the kernel two-sample test's sums on the GPU box (no fallback: needs the MI355X).  Writes
profiles/mmd_timing.txt (--out) and prints one JSON line.

n_x = n_y = 5000 and 2500 rows of seeded Gaussian latents (the second set's mean moved by 0.1), D = 32 and 64, P = 1000
relabellings drawn as ops.mmd_draw draws them, the Gaussian family with the five default widths and the energy kernel.
ops.mmd_sums -- the member check and all seven launches, the relabellings already on the device -- against the same
sums composed from torch-ROCm float64 ops on the same GPU, never an earlier run of this code: cdist of the pooled rows
(its default mode, the Gram form: compute_mode="donot_use_mm_for_euclid_dist" returned wrong distances at these sizes),
the kernel function, fill_diagonal_, one (1 + P, n) x (n, n) matmul A @ K, and sxx = (A @ K * A).sum(1), sxy =
(A @ K * (1 - A)).sum(1), syy = T - sxx - 2 sxy.  Both sides warmed, alternated, three times each; device events
around whole calls that end in a synchronise; the peak of the caching allocator over one call of each side.  Reported
with the largest deviation of the sums relative to the sum of |k|; reported, not gated."""
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
P, SEED, RUNS = 1000, 0, 3
SHAPES = [(5000, 32), (5000, 64), (2500, 32), (2500, 64)]
KERNELS = ["rbf", "energy"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    del out
    return peak


def torch_sums(X, Y, member, kernel, params):
    """the composed route: (1 + P, 3) float64 and the (n,) row sums"""
    Z = torch.cat([X, Y]).double()
    d = torch.cdist(Z, Z)
    if kernel == "energy":
        K = -d
    else:
        d2 = d * d
        K = sum(torch.exp(-p * d2) for p in params) / len(params)
    K.fill_diagonal_(0.0)
    first = torch.zeros(1, Z.shape[0], dtype=torch.float64, device=Z.device)
    first[0, :X.shape[0]] = 1.0
    A = torch.cat([first, member.double()])
    AK = A @ K
    rows = K.sum(1)
    sxx, sxy = (AK * A).sum(1), (AK * (1.0 - A)).sum(1)
    return torch.stack([sxx, rows.sum() - sxx - 2.0 * sxy, sxy], 1), rows


def bench(n_half, D, kernel):
    rs = np.random.RandomState(11)
    X = torch.from_numpy(rs.standard_normal((n_half, D)).astype(np.float32)).to(DEV)
    Y = torch.from_numpy((rs.standard_normal((n_half, D)) + 0.1).astype(np.float32)).to(DEV)
    member = torch.from_numpy(ops.mmd_draw(n_half, n_half, P, SEED)).to(DEV)
    # the widths of the whole sample, computed once: both sides take the same numbers
    params = () if kernel == "energy" else ops.mmd_sums(X, Y, kernel=kernel)[2]
    hip = lambda: ops.mmd_sums(X, Y, member, kernel=kernel, params=params)[:2]      # noqa: E731
    composed = lambda: torch_sums(X, Y, member, kernel, params)      # noqa: E731
    for _ in range(2):      # warm-up of every shape both sides use (first calls include code loading)
        hip()
        composed()
    n = 2 * n_half
    res = {"n_x": n_half, "n_y": n_half, "D": D, "P": P, "kernel": kernel, "scales": len(params),
           "chunks": ops.H.lib().mmvae_mmd_chunks(n), "hip_ms": [], "torch_ms": []}
    for _ in range(RUNS):
        t, out_t = timed(composed)
        res["torch_ms"].append(t)
        t, out_h = timed(hip)
        res["hip_ms"].append(t)
    scale = torch_sums(X, Y, member[:0], kernel, params)[1].abs().sum()      # sum of |k| (one sign per family)
    res["sums_dev"] = float((out_h[0] - out_t[0]).abs().max() / scale)
    res["rows_dev"] = float(((out_h[1] - out_t[1]).abs() / out_t[1].abs()).max())
    est = ops.mmd2_from_sums(out_h[0], n_half, n_half)
    res["mmd2"], res["p_value"] = float(est[0]), (1 + int((est[1:] >= est[0]).sum())) / (1 + P)
    del out_t, out_h
    res["hip_peak_mib"], res["torch_peak_mib"] = peak_mib(hip), peak_mib(composed)
    # the arithmetic of the HIP route: per block of columns every tile's Gram product (2 D flops a pair) and its product
    # with the block of indicators (2 x 128 flops a pair)
    blocks = -(-(P + ops.H.MMD_EXTRA_COLUMNS) // ops.H.MMD_PBLOCK)
    tiles = -(-n // 64)
    res["mfma_gflop"] = blocks * tiles * tiles * 64 * 64 * 2 * (D + ops.H.MMD_PBLOCK) / 1e9
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmd_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mmd.py needs the MI355X"
    res = []
    for n_half, D in SHAPES:
        for kernel in KERNELS:
            res.append(bench(n_half, D, kernel))
            print(f"n {2 * n_half} D {D} {kernel} done", file=sys.stderr, flush=True)
    lines = [f"Kernel two-sample test, the sums of the observed split and P = {P} relabellings, one MI355X "
             f"(tools/bench_mmd.py): float64, best of {RUNS} warmed, alternated runs; device events around whole calls.  HIP = "
             "ops.mmd_sums (the member check and seven launches; the n x n matrix is never written); torch-ROCm composed = "
             "cdist, the kernel function, one (1 + P, n) x (n, n) float64 matmul and row-wise products.  Peak = the caching "
             "allocator's high-water mark over one call, beside the inputs", ""]
    for r in res:
        h, t = min(r["hip_ms"]), min(r["torch_ms"])
        lines.append(f"n_x = n_y = {r['n_x']}, D {r['D']}, {r['kernel']} ({r['scales']} widths; {r['chunks']} column chunk(s) per "
                     f"row tile):")
        lines.append(f"  HIP {h:.1f} ms  torch-ROCm composed {t:.1f} ms  HIP/torch {h / t:.2f}  (runs: HIP "
                     f"{[round(x, 1) for x in r['hip_ms']]}, torch {[round(x, 1) for x in r['torch_ms']]})")
        lines.append(f"  peak memory: HIP {r['hip_peak_mib']:.0f} MiB, torch {r['torch_peak_mib']:.0f} MiB;  "
                     f"{r['mfma_gflop']:.0f} GFLOP of fp64 tile products: {r['mfma_gflop'] / h:.1f} TFLOP/s over the whole call")
        lines.append(f"  the sums deviate {r['sums_dev']:.1e} of sum |k| at the most, the row sums {r['rows_dev']:.1e} relative; "
                     f"mmd2 {r['mmd2']:.6g}, p {r['p_value']:.4g}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
