"""Timing of the Frechet distance on the GPU box (no fallback: needs the MI355X).  Writes profiles/frechet_timing.txt (--out)
and prints one JSON line.

F = 50 (the digit classifiers' hidden layer), 512 (the attribute classifiers' trunk) and 2048 (pooled Inception features)
at N = 10 000 rows per set of seeded relu features.  Reported separately: the streaming moments (10 batches of 1000 rows per
set), each of the two eigendecompositions with its sweep count, and the whole distance -- against two baselines, never an
earlier run of this code: the same route composed from torch-ROCm ops in float64 on the same GPU (torch.cov,
torch.linalg.eigh, matmul), and the reference's own arithmetic on this box's CPU (np.cov + scipy.linalg.sqrtm, with the
thread count the process is given; one run, seconds at F = 2048).  GPU sides warmed, alternated, twice each;
device events around whole calls that end in a synchronise.  Reported, not gated."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from multimodal_vae_comparison_amd import ops

DEV = "cuda"
N = 10000
BATCH = 1000


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def data(F, seed):
    rs = np.random.RandomState(seed)
    W = rs.standard_normal((F, F)) / np.sqrt(F)
    X = np.maximum((0.2 * seed + rs.standard_normal((N, F))) @ W + 0.5 * rs.standard_normal(F), 0.0)
    return torch.from_numpy(X.astype(np.float32)).to(DEV)


def hip_moments(X):
    st = ops.frechet_state(X.shape[1], DEV)
    for lo in range(0, N, BATCH):
        ops.frechet_update(st, X[lo:lo + BATCH])
    return ops.frechet_moments(st)[1:]


def torch_moments(X):
    X = X.double()
    return X.mean(0), torch.cov(X.T)


def torch_distance(mu1, s1, mu2, s2):
    lam, V = torch.linalg.eigh(s1)
    R = lam.clamp_min(0.0).sqrt()[:, None] * V.T
    G = R @ s2 @ R.T
    tr = torch.linalg.eigvalsh(0.5 * (G + G.T)).clamp_min(0.0).sqrt().sum()
    d = mu1 - mu2
    return float(d @ d + s1.trace() + s2.trace() - 2.0 * tr)


def cpu_reference(X1, X2):
    try:
        from scipy import linalg
    except ImportError:
        return None, None
    X1, X2 = X1.cpu().numpy().astype(np.float64), X2.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    mu1, s1, mu2, s2 = X1.mean(0), np.cov(X1, rowvar=False), X2.mean(0), np.cov(X2, rowvar=False)
    covmean = linalg.sqrtm(s1.dot(s2), disp=False)[0]
    d = mu1 - mu2
    val = float(d.dot(d) + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(covmean.real))
    return 1e3 * (time.perf_counter() - t0), val


def bench(F, cpu=True):
    X1, X2 = data(F, 1), data(F, 2)
    for _ in range(2):      # warm-up of every shape both sides use (first calls include code loading)
        mu1, s1 = hip_moments(X1)
        mu2, s2 = hip_moments(X2)
        tm1, ts1 = torch_moments(X1)
    ops.frechet_distance(mu1, s1, mu2, s2)
    torch_distance(mu1, s1, mu2, s2)
    res = {"F": F, "N": N, "waves_per_pair": ops.H.lib().mmvae_sym_eig_waves_per_pair(F), "hip_moments_ms": [],
           "torch_moments_ms": [], "hip_distance_ms": [], "torch_distance_ms": [], "hip_eig1_ms": [], "hip_eig2_ms": []}
    lam = ops.sym_eig(s1)
    R = lam["values"].sqrt()[:, None] * lam["vectors"].t()
    G = ops.f64_gemm(R, ops.f64_gemm(s2, R, trans_b=True))
    for _ in range(2):
        res["torch_moments_ms"].append(timed(lambda: torch_moments(X1))[0])
        res["hip_moments_ms"].append(timed(lambda: hip_moments(X1))[0])
        t, dt = timed(lambda: torch_distance(mu1, s1, mu2, s2))
        res["torch_distance_ms"].append(t)
        t, out = timed(lambda: ops.frechet_distance(mu1, s1, mu2, s2))
        res["hip_distance_ms"].append(t)
        t, e1 = timed(lambda: ops.sym_eig(s1))
        res["hip_eig1_ms"].append(t)
        t, e2 = timed(lambda: ops.sym_eig(G, vectors=False))
        res["hip_eig2_ms"].append(t)
    res.update(sweeps=list(out["sweeps"]), eig_sweeps=[e1["sweeps"], e2["sweeps"]], d_hip=float(out["distance"]), d_torch=dt,
               moments_dev=float((s1 - ts1).abs().max() / ts1.diagonal().max()),
               threads=torch.get_num_threads())
    res["cpu_reference_ms"], res["d_cpu"] = cpu_reference(X1, X2) if cpu else (None, None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frechet_timing.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[50, 512, 2048])
    ap.add_argument("--no-cpu", action="store_true", help="skip the scipy.linalg.sqrtm baseline")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frechet.py needs the MI355X"
    res = []
    for F in args.sizes:
        res.append(bench(F, cpu=not args.no_cpu))
        print(f"F {F} done", file=sys.stderr, flush=True)
    lines = [f"Frechet distance, one MI355X (tools/bench_frechet.py): N = {N} rows per set, float64, best of two warmed, "
             "alternated runs; device events around whole calls", ""]
    for r in res:
        steps = r["F"] + (r["F"] & 1) - 1
        cpu = "not run" if r["cpu_reference_ms"] is None else \
            f"{r['cpu_reference_ms']:.0f} ms on {r['threads']} threads (d^2 deviates {abs(r['d_hip'] - r['d_cpu']) / abs(r['d_cpu']):.1e})"
        lines += [f"F {r['F']}: moments of one set (10 batches of {BATCH}) HIP {min(r['hip_moments_ms']):.2f} ms  torch.cov float64 "
                  f"{min(r['torch_moments_ms']):.2f} ms  (covariance deviates {r['moments_dev']:.1e} of the largest variance)",
                  f"  eigendecomposition of sigma1: {min(r['hip_eig1_ms']):.1f} ms, {r['eig_sweeps'][0]} sweeps of {steps} launches, "
                  f"{r['waves_per_pair']} wave(s) per pair; of G (values only): {min(r['hip_eig2_ms']):.1f} ms, "
                  f"{r['eig_sweeps'][1]} sweeps",
                  f"  whole distance: HIP {min(r['hip_distance_ms']):.1f} ms (sweeps {r['sweeps']})  torch-ROCm composed (eigh, "
                  f"matmul) {min(r['torch_distance_ms']):.1f} ms  HIP/torch {min(r['hip_distance_ms']) / min(r['torch_distance_ms']):.2f}"
                  f"  (runs: HIP {[round(t, 1) for t in r['hip_distance_ms']]}, torch {[round(t, 1) for t in r['torch_distance_ms']]}; "
                  f"d^2 HIP {r['d_hip']:.10g}, torch {r['d_torch']:.10g})",
                  f"  reference arithmetic on the CPU (np.cov + scipy.linalg.sqrtm, moments included): {cpu}"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
