"""Timing of precision / recall / density / coverage on the GPU box (no fallback: needs the MI355X).  Writes
profiles/manifold_timing.txt (--out) and prints one JSON line.

F = 50 (the digit classifiers' hidden layer), 512 (the attribute classifiers' trunk) and 2048 (pooled Inception features)
at N = M = 10 000 rows of seeded relu features (the generator of tests/manifold_reference.py, restated), k = 5.  Reported
separately: the two radii passes, the two cross passes (each op call with its squared norms) and the whole manifold_prdc --
against two baselines, never an earlier run of this code: the same quantities composed from torch-ROCm ops in float64 on
the same GPU (Gram form: norms, one matmul, clamp; kthvalue for the radii, comparisons and min for the cross pass; the N x M
float64 temporary is 800 MB and is not blocked; the whole composed prdc forms the real-generated matrix once and reads it
in both orientations: three products where the kernels run four), and a numpy float64 run of that route on this box's CPU
(one run, with the thread count the process is given).  GPU sides warmed, alternated, twice each; device events around
whole calls that end in a synchronise.  Reported, not gated."""
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
K = 5
SCALARS = ("precision", "recall", "density", "coverage")


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


# ---- the composed route, torch float64 on the GPU ------------------------------------------------------------------------------
def torch_sqdist(B, A):
    B, A = B.double(), A.double()
    return ((B * B).sum(1)[:, None] + (A * A).sum(1)[None, :] - 2.0 * (B @ A.T)).clamp_min_(0.0)


def torch_radii(X, k=K):
    D = torch_sqdist(X, X)
    D.fill_diagonal_(float("inf"))
    return D.kthvalue(k, dim=1).values


def torch_cross(B, A, rad2):
    D = torch_sqdist(B, A)
    return (D <= rad2[None, :]).sum(1), D.min(1).values


def torch_prdc(R, G, k=K):
    rad_r, rad_g = torch_radii(R, k), torch_radii(G, k)
    D = torch_sqdist(G, R)
    hit_r, hit_g, near_r = (D <= rad_r[None, :]).sum(1), (D.T <= rad_g[None, :]).sum(1), D.min(0).values
    return {"precision": int((hit_r > 0).sum()) / len(G), "recall": int((hit_g > 0).sum()) / len(R),
            "density": int(hit_r.sum()) / (k * len(G)), "coverage": int((near_r <= rad_r).sum()) / len(R)}


# ---- the same route, numpy float64 on the CPU ------------------------------------------------------------------------------------
def numpy_prdc(R, G, k=K):
    t0 = time.perf_counter()
    R, G = R.astype(np.float64), G.astype(np.float64)
    nr, ng = (R * R).sum(1), (G * G).sum(1)

    def radii(X, n2):
        D = np.maximum(n2[:, None] + n2[None, :] - 2.0 * (X @ X.T), 0.0)
        np.fill_diagonal(D, np.inf)
        return np.partition(D, k - 1, axis=1)[:, k - 1]

    rad_r, rad_g = radii(R, nr), radii(G, ng)
    D = np.maximum(ng[:, None] + nr[None, :] - 2.0 * (G @ R.T), 0.0)
    hit_r, hit_g, near_r = (D <= rad_r[None, :]).sum(1), (D.T <= rad_g[None, :]).sum(1), D.min(0)
    out = {"precision": int((hit_r > 0).sum()) / len(G), "recall": int((hit_g > 0).sum()) / len(R),
           "density": int(hit_r.sum()) / (k * len(G)), "coverage": int((near_r <= rad_r).sum()) / len(R)}
    return 1e3 * (time.perf_counter() - t0), out


def bench(F, cpu=True):
    Rn, Gn = data(F, 1), data(F, 2, 0.05, 1.0)
    R, G = torch.from_numpy(Rn).to(DEV), torch.from_numpy(Gn).to(DEV)
    for _ in range(2):      # warm-up of every shape both sides use (first calls include code loading)
        rad_r, rad_g = ops.manifold_radii(R, K), ops.manifold_radii(G, K)
        ops.manifold_cross(G, R, rad_r)
        ops.manifold_cross(R, G, rad_g)
        ops.manifold_prdc(R, G, k=K)
        torch_cross(G, R, torch_radii(R))
        torch_prdc(R, G)
    res = {"F": F, "N": N, "k": K, "chunks": ops.H.lib().mmvae_manifold_chunks(N, N)}
    parts = {"radii_real": (lambda: ops.manifold_radii(R, K), lambda: torch_radii(R)),
             "radii_fake": (lambda: ops.manifold_radii(G, K), lambda: torch_radii(G)),
             "cross_fake_in_real": (lambda: ops.manifold_cross(G, R, rad_r), lambda: torch_cross(G, R, rad_r)),
             "cross_real_in_fake": (lambda: ops.manifold_cross(R, G, rad_g), lambda: torch_cross(R, G, rad_g)),
             "prdc": (lambda: ops.manifold_prdc(R, G, k=K), lambda: torch_prdc(R, G))}
    for name, (hip, composed) in parts.items():
        res[f"hip_{name}_ms"], res[f"torch_{name}_ms"] = [], []
        for _ in range(2):
            t, out_t = timed(composed)
            res[f"torch_{name}_ms"].append(t)
            t, out_h = timed(hip)
            res[f"hip_{name}_ms"].append(t)
    res["hip"] = {n: out_h[n] for n in SCALARS}
    res["torch"] = out_t
    res["rad2_dev"] = float(((ops.manifold_radii(R, K) - torch_radii(R)).abs() / torch_radii(R)).max())
    res["threads"] = torch.get_num_threads()
    res["numpy_prdc_ms"], res["numpy"] = numpy_prdc(Rn, Gn) if cpu else (None, None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manifold_timing.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[50, 512, 2048])
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy baseline")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_manifold.py needs the MI355X"
    res = []
    for F in args.sizes:
        res.append(bench(F, cpu=not args.no_cpu))
        print(f"F {F} done", file=sys.stderr, flush=True)
    lines = [f"Precision / recall / density / coverage, one MI355X (tools/bench_manifold.py): N = M = {N} rows, k = {K}, float64 "
             "distances, best of two warmed, alternated runs; device events around whole calls.  torch-ROCm composed = Gram "
             "form in float64 with one unblocked 800 MB N x M temporary, kthvalue / comparisons / min; its whole prdc forms "
             "three products, the kernels four", ""]
    for r in res:
        best = lambda key: min(r[key])      # noqa: E731
        lines.append(f"F {r['F']} ({r['chunks']} column chunks per row tile):")
        for name, label in (("radii_real", "radii of the real set"), ("radii_fake", "radii of the generated set"),
                            ("cross_fake_in_real", "cross pass, generated rows in real spheres"),
                            ("cross_real_in_fake", "cross pass, real rows in generated spheres"), ("prdc", "whole manifold_prdc")):
            h, t = best(f"hip_{name}_ms"), best(f"torch_{name}_ms")
            lines.append(f"  {label}: HIP {h:.1f} ms  torch-ROCm composed {t:.1f} ms  HIP/torch {h / t:.2f}  (runs: HIP "
                         f"{[round(x, 1) for x in r[f'hip_{name}_ms']]}, torch {[round(x, 1) for x in r[f'torch_{name}_ms']]})")
        same = "the same four numbers" if r["hip"] == r["torch"] else f"torch gives {r['torch']}"
        lines.append("  " + ", ".join(f"{n} {r['hip'][n]:.6g}" for n in SCALARS) + f" ({same}; rad^2 deviates "
                     f"{r['rad2_dev']:.1e} relative)")
        cpu = "not run" if r["numpy_prdc_ms"] is None else \
            (f"{r['numpy_prdc_ms']:.0f} ms on {r['threads']} threads, "
             + ("the same four numbers" if r["numpy"] == r["hip"] else f"giving {r['numpy']}"))
        lines.append(f"  numpy float64 on the CPU (Gram form, np.partition), whole prdc: {cpu}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
