"""Timing of the latent density estimation on the GPU box (no fallback: needs the MI355X).  Writes profiles/gmm_timing.txt
(--out) and prints one JSON line.

ops.gmm_fit at N = 10 000 rows, C = 10 components, R = 10 restarts, D = 32 and 64 (latent widths), full and diagonal
covariances, tol = 0 and max_iter = 20: every restart runs exactly 20 iterations and the final E-step.  Seeded blobs (the
generator of tests/gmm_reference.py, restated: centres 3 N(0, 1), unit noise, start labels = the truth with 20 % moved to
the next id, another 20 % per restart) -- against the same EM composed from torch-ROCm float64 ops on the same GPU, never an
earlier run of this code: one-hot start, batched matmuls for the moments and the centred covariances, torch.linalg.cholesky,
solve_triangular against the identity, a batched matmul for (x - mu) P, torch.logsumexp; all restarts as one batch, no host
synchronisation inside the 20 iterations.
GPU sides warmed, alternated, three times each; device events around whole calls that end in a synchronise.  Reported, not
gated."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from multimodal_vae_comparison_amd import ops

DEV = "cuda"
N, C, R, ITERS, REG = 10000, 10, 10, 20, 1e-6


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def data(D, seed):
    rs = np.random.RandomState(seed)
    centres = 3.0 * rs.standard_normal((C, D))
    of = np.arange(N) % C
    X = (centres[of] + rs.standard_normal((N, D))).astype(np.float32)
    starts = np.stack([np.where(rs.random_sample(N) < 0.2, (of + 1) % C, of) for _ in range(R)]).astype(np.int32)
    return X, starts


# ---- the composed route, torch float64 on the GPU ---------------------------------------------------------------------------------
def torch_em(X, starts, kind, iters=ITERS, reg=REG):
    X64 = X.double()
    D = X64.shape[1]
    eye = torch.eye(D, dtype=torch.float64, device=X.device)
    tiny = 10.0 * float(np.finfo(np.float64).eps)

    def m_step(resp):      # resp (R, N, C)
        rt = resp.transpose(1, 2)      # (R, C, N)
        nk = resp.sum(1) + tiny
        means = rt @ X64 / nk[:, :, None]
        if kind == "full":
            diff = X64[None, None] - means[:, :, None, :]      # (R, C, N, D)
            cov = (rt[:, :, :, None] * diff).transpose(2, 3) @ diff / nk[:, :, None, None] + reg * eye
            L = torch.linalg.cholesky(cov)
            P = torch.linalg.solve_triangular(L, eye.expand_as(L), upper=False).transpose(2, 3)
            logdet = P.diagonal(dim1=2, dim2=3).log().sum(2)
        else:
            cov = rt @ (X64 * X64) / nk[:, :, None] - means ** 2 + reg
            P = cov.rsqrt()
            logdet = P.log().sum(2)
        w = nk / N
        return w / w.sum(1, keepdim=True), means, cov, P, logdet

    def e_step(w, means, P, logdet):
        diff = X64[None, None] - means[:, :, None, :]
        y = diff @ P if kind == "full" else diff * P[:, :, None, :]
        lp = -0.5 * (D * math.log(2.0 * math.pi) + (y * y).sum(3)) + (logdet + w.log())[:, :, None]      # (R, C, N)
        norm = torch.logsumexp(lp, 1)
        return norm, lp, (lp - norm[:, None, :]).exp().transpose(1, 2)

    w, means, cov, P, logdet = m_step(torch.nn.functional.one_hot(starts.long(), C).double())
    bound = None
    for _ in range(iters):
        norm, _, resp = e_step(w, means, P, logdet)
        w, means, cov, P, logdet = m_step(resp)
        bound = norm.mean(1)
    norm, lp, resp = e_step(w, means, P, logdet)
    return {"weights": w, "means": means, "covariances": cov, "lower_bound": bound, "labels": lp.argmax(1), "log_density": norm}


def bench(D, kind):
    X, starts = (torch.from_numpy(a).to(DEV) for a in data(D, 1))
    hip = lambda: ops.gmm_fit(X, starts, covariance_type=kind, reg_covar=REG, tol=0.0, max_iter=ITERS, n_components=C)
    composed = lambda: torch_em(X, starts, kind)
    for _ in range(2):      # warm-up of every shape both sides use (first calls include code loading)
        hip()
        composed()
    ms = {"hip": [], "torch": []}
    for _ in range(3):
        t, out_t = timed(composed)
        ms["torch"].append(t)
        t, out_h = timed(hip)
        ms["hip"].append(t)
    assert out_h["n_iter"].tolist() == [ITERS] * R and not bool(out_h["degenerate"].any())
    return {"D": D, "kind": kind, "hip_ms": ms["hip"], "torch_ms": ms["torch"],
            "labels_differ": int((out_h["labels"].long() != out_t["labels"]).sum()),
            "bound_dev": float((out_h["lower_bound"] - out_t["lower_bound"]).abs().max()),
            "means_dev": float((out_h["means"] - out_t["means"]).abs().max()),
            "covariances_dev": float((out_h["covariances"] - out_t["covariances"]).abs().max()),
            "bound": out_h["lower_bound"].tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm_timing.txt"))
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gmm.py needs the MI355X"
    runs = [bench(D, kind) for D in args.dims for kind in ("full", "diag")]
    lines = [f"Latent density estimation, one MI355X (tools/bench_gmm.py): N = {N} rows, C = {C} components, {R} restarts, tol = 0, "
             f"{ITERS} iterations and the final E-step, float64, best of three warmed, alternated runs; device events around "
             "whole calls.  torch-ROCm composed = one-hot start, batched matmuls, linalg.cholesky, solve_triangular, logsumexp "
             "in float64, all restarts as one batch", ""]
    for r in runs:
        h, t = min(r["hip_ms"]), min(r["torch_ms"])
        lines.append(f"gmm_fit, D {r['D']}, {r['kind']}: HIP {h:.1f} ms  torch-ROCm composed {t:.1f} ms  HIP/torch {h / t:.2f}  "
                     f"(runs: HIP {[round(x, 1) for x in r['hip_ms']]}, torch {[round(x, 1) for x in r['torch_ms']]}; "
                     f"{r['labels_differ']} labels differ, bound deviates {r['bound_dev']:.1e}, means {r['means_dev']:.1e}, "
                     f"covariances {r['covariances_dev']:.1e})")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps({"gmm": runs}))


if __name__ == "__main__":
    main()
