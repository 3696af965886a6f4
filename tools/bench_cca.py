"""Timing of the cross-modal correlation on the GPU box (no fallback: needs the MI355X).  Writes profiles/cca_timing.txt
(--out) and prints one JSON line.

Two views of 512 and 300 features (an image trunk beside a sentence embedding), 10 000 rows of seeded latent-factor data, k
joint dimensions.  Reported separately: the streaming moments at O = 812 (10 batches of 1000 rows), the fit from the moments
(ops.cca_fit: three Jacobi eigendecompositions and the block products) and the score of 10 000 pairs (ops.cca_score) --
each against the same outputs composed from torch-ROCm float64 ops on the same GPU (torch.cov; torch.linalg.eigh per view
and of the whitened matrix, matmul; centred matmuls and a cosine), never against an earlier run of this code.  GPU sides
warmed, alternated, twice each; device events around whole calls that end in a synchronise.  Reported, not gated."""
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
BATCH = 1000


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def data(widths, rows, seed):
    rs = np.random.RandomState(seed)
    d = 32
    z = rs.standard_normal((rows, d)) * np.geomspace(3.0, 0.3, d)
    return [torch.from_numpy((z @ (rs.standard_normal((d, o)) / np.sqrt(d)) + rs.standard_normal((rows, o)))
                             .astype(np.float32)).to(DEV) for o in widths]


def hip_moments(X):
    st = ops.frechet_state(X.shape[1], DEV)
    for lo in range(0, X.shape[0], BATCH):
        ops.frechet_update(st, X[lo:lo + BATCH])
    return ops.frechet_moments(st)[1:]


def torch_moments(X):
    X = X.double()
    return X.mean(0), torch.cov(X.T)


def torch_fit(sigma, widths, k, ridge):
    O = sigma.shape[0]
    offs = np.concatenate([[0], np.cumsum(widths)])
    W = torch.zeros_like(sigma)
    eye = torch.eye(O, dtype=torch.float64, device=sigma.device)
    for lo, hi in zip(offs[:-1], offs[1:]):
        lam, Q = torch.linalg.eigh(sigma[lo:hi, lo:hi] + ridge * eye[lo:hi, lo:hi])
        W[lo:hi, lo:hi] = (Q * lam.rsqrt()) @ Q.T
    N = W @ (sigma + 2.0 * ridge * eye) @ W
    values, vectors = torch.linalg.eigh(0.5 * (N + N.T))
    order = torch.sort(values, descending=True, stable=True).indices[:k]
    P = W @ vectors[:, order]
    return values[order] - 1.0, P / torch.linalg.vector_norm(P, dim=0, keepdim=True)


def torch_score(a, b, ma, mb, Pa, Pb):
    p, q = (a.double() - ma) @ Pa, (b.double() - mb) @ Pb
    cos = (p * q).sum(1) / (torch.linalg.vector_norm(p, dim=1).clamp_min(1e-8) * torch.linalg.vector_norm(q, dim=1).clamp_min(1e-8))
    return cos, cos.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cca_timing.txt"))
    ap.add_argument("--widths", type=int, nargs="+", default=[512, 300])
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--ridge", type=float, default=1e-12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cca.py needs the MI355X"
    widths, k = list(args.widths), args.k
    views = data(widths, args.rows, 1)
    X = torch.cat(views, 1)
    res = {"widths": widths, "rows": args.rows, "k": k, "ridge": args.ridge}
    for key in ("hip_moments_ms", "torch_moments_ms", "hip_fit_ms", "torch_fit_ms", "hip_score_ms", "torch_score_ms"):
        res[key] = []
    mu, sigma = hip_moments(X)      # warm-up of every shape both sides use (first calls include code loading)
    torch_moments(X)
    fit = ops.cca_fit(mu, sigma, widths, k, args.ridge)
    tv, tP = torch_fit(sigma, widths, k, args.ridge)
    score_args = (views[0], views[1], fit["means"][0], fit["means"][1], fit["projections"][0], fit["projections"][1])
    ops.cca_score(*score_args)
    torch_score(*score_args)
    for _ in range(2):
        res["torch_moments_ms"].append(timed(lambda: torch_moments(X))[0])
        res["hip_moments_ms"].append(timed(lambda: hip_moments(X))[0])
        res["torch_fit_ms"].append(timed(lambda: torch_fit(sigma, widths, k, args.ridge))[0])
        t, fit = timed(lambda: ops.cca_fit(mu, sigma, widths, k, args.ridge))
        res["hip_fit_ms"].append(t)
        t, (tcos, tsum) = timed(lambda: torch_score(*score_args))
        res["torch_score_ms"].append(t)
        t, (cos, total) = timed(lambda: ops.cca_score(*score_args))
        res["hip_score_ms"].append(t)
    P = torch.cat(fit["projections"], 0)
    sign = torch.sign((P * tP).sum(0))
    res.update(sweeps=fit["sweeps"], condition=fit["condition"],
               values_dev=float((fit["correlations"] - tv).abs().max()), projections_dev=float((P * sign - tP).abs().max()),
               score_dev=float((cos - tcos).abs().max()), mean_score=float(total) / args.rows, first=float(fit["correlations"][0]),
               last=float(fit["correlations"][-1]))
    best = {key: min(v) for key, v in res.items() if key.endswith("_ms")}
    O = sum(widths)
    lines = [f"Cross-modal correlation, one MI355X (tools/bench_cca.py): views of {widths} features (O = {O}), {args.rows} rows, "
             f"k = {k}, ridge {args.ridge:g}, float64, best of two warmed, alternated runs; device events around whole calls", "",
             f"moments at O = {O} ({args.rows // BATCH} batches of {BATCH}): HIP {best['hip_moments_ms']:.2f} ms  torch.cov float64 "
             f"{best['torch_moments_ms']:.2f} ms",
             f"fit from the moments: HIP {best['hip_fit_ms']:.1f} ms (Jacobi sweeps: views {res['sweeps']['views']}, whitened "
             f"matrix {res['sweeps']['joint']})  torch-ROCm composed (eigh, matmul) {best['torch_fit_ms']:.1f} ms  HIP/torch "
             f"{best['hip_fit_ms'] / best['torch_fit_ms']:.2f}  (runs: HIP {[round(t, 1) for t in res['hip_fit_ms']]}, torch "
             f"{[round(t, 1) for t in res['torch_fit_ms']]})",
             f"  correlations {res['first']:.6f} .. {res['last']:.6f}; against the torch composition: values {res['values_dev']:.1e}, "
             f"projections {res['projections_dev']:.1e}; lambda_min / lambda_max of the views {[f'{c:.2e}' for c in res['condition']]}",
             f"score of {args.rows} pairs: HIP {best['hip_score_ms']:.3f} ms  torch-ROCm composed (centred matmuls, cosine) "
             f"{best['torch_score_ms']:.3f} ms  HIP/torch {best['hip_score_ms'] / best['torch_score_ms']:.2f}  (runs: HIP "
             f"{[round(t, 3) for t in res['hip_score_ms']]}, torch {[round(t, 3) for t in res['torch_score_ms']]}; rows deviate "
             f"{res['score_dev']:.1e}; mean score {res['mean_score']:.6f})"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
