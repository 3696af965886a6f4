"""Timing of the latent cluster analysis on the GPU box (no fallback: needs the MI355X).  Writes
profiles/cluster_timing.txt (--out) and prints one JSON line.

kmeans_fit at N = 10 000 rows, C = 10 clusters, R = 10 restarts, D = 32 and 64 (latent widths), and silhouette at N = 10 000,
F = 64 and 512, on seeded overlapping blobs (the generator of tests/cluster_reference.py, restated) -- against the same
outputs composed from torch-ROCm ops in float64 on the same GPU, never an earlier run of this code:
  k-means     per iteration cdist of the rows against the (R, C, D) centres, argmin, one-hot masked sums as a batched matmul,
              where() for the clusters without rows; all restarts iterate until the host, which looks every
              KMEANS_CHECK_EVERY iterations as the op does, finds no label of any restart changed; a last cdist for
              the inertia.  (Past its convergence a restart is at a fixed point: the same labels and centres.)
  silhouette  cdist of the rows against themselves (one unblocked 800 MB N x N float64 temporary), the diagonal zeroed, one
              matmul with the one-hot labels, the same final row arithmetic.
GPU sides warmed, alternated, twice each; device events around whole calls that end in a synchronise.  Reported, not gated."""
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
N, C, R = 10000, 10, 10


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
    centres = rs.standard_normal((C, F))
    return (centres[np.arange(N) % C] + np.sqrt(2.0 * F) / 4.0 * rs.standard_normal((N, F))).astype(np.float32)


# ---- the composed routes, torch float64 on the GPU --------------------------------------------------------------------------------
def torch_kmeans(X, init, max_iter=300):
    X64 = X.double()
    mu = X64[init.long()]
    batch = X64[None].expand(len(mu), -1, -1)
    prev = torch.full((len(mu), len(X)), -1, device=X.device)
    n_iter = torch.zeros(len(mu), dtype=torch.int64, device=X.device)
    done = torch.zeros(len(mu), dtype=torch.bool, device=X.device)
    for t in range(1, max_iter + 1):
        lab = torch.cdist(batch, mu).argmin(2)
        same = (lab == prev).all(1)
        n_iter = torch.where(done, n_iter, torch.full_like(n_iter, t))
        done = done | same
        onehot = torch.nn.functional.one_hot(lab, C).double()
        counts = onehot.sum(1)
        mu = torch.where(((counts > 0) & ~done[:, None])[:, :, None], (onehot.transpose(1, 2) @ batch) / counts.clamp(min=1)[:, :, None], mu)
        prev = lab
        if t % ops.KMEANS_CHECK_EVERY == 0 and bool(done.all()):
            break
    d = torch.cdist(batch, mu)
    lab = d.argmin(2)
    return {"centres": mu, "labels": lab, "inertia": (d.min(2).values ** 2).sum(1), "n_iter": n_iter, "converged": done}


def torch_silhouette(X, labels):
    X64, lab = X.double(), labels.long()
    D = torch.cdist(X64, X64)
    D.fill_diagonal_(0.0)
    onehot = torch.nn.functional.one_hot(lab, C).double()
    cnt = onehot.sum(0)
    S = D @ onehot
    own = cnt[lab]
    a = S.gather(1, lab[:, None])[:, 0] / (own - 1).clamp(min=1)
    others = (cnt[None, :] > 0) & (torch.arange(C, device=X.device)[None, :] != lab[:, None])
    b = torch.where(others, S / cnt.clamp(min=1)[None, :], torch.full_like(S, float("inf"))).min(1).values
    top = torch.maximum(a, b)
    s = torch.where((own > 1) & (top > 0), (b - a) / top, torch.zeros_like(top))
    return {"samples": s, "score": float(s.mean()), "sums": S}


def alternate(hip, composed):
    ms = {"hip": [], "torch": []}
    for _ in range(2):
        t, out_t = timed(composed)
        ms["torch"].append(t)
        t, out_h = timed(hip)
        ms["hip"].append(t)
    return ms, out_h, out_t


def bench_kmeans(D):
    X = torch.from_numpy(data(D, 1)).to(DEV)
    init = torch.from_numpy(ops.kmeans_draw(N, C, R, 0)).to(DEV)
    for _ in range(2):      # warm-up of every shape both sides use (first calls include code loading)
        ops.kmeans_fit(X, init)
        torch_kmeans(X, init)
    ms, h, t = alternate(lambda: ops.kmeans_fit(X, init), lambda: torch_kmeans(X, init))
    return {"D": D, "hip_ms": ms["hip"], "torch_ms": ms["torch"], "n_iter": h["n_iter"].tolist(), "torch_n_iter": t["n_iter"].tolist(),
            "labels_differ": int((h["labels"].long() != t["labels"]).sum()),
            "inertia_dev": float(((h["inertia"] - t["inertia"]).abs() / t["inertia"]).max()), "best": h["best"]}


def bench_silhouette(F):
    X = torch.from_numpy(data(F, 2)).to(DEV)
    labels = (torch.arange(N, device=DEV) % C).to(torch.int32)
    for _ in range(2):
        ops.silhouette(X, labels, C)
        torch_silhouette(X, labels)
    ms, h, t = alternate(lambda: ops.silhouette(X, labels, C), lambda: torch_silhouette(X, labels))
    tiles = int(((h["counts"].cpu().numpy() + 63) // 64).sum())
    return {"F": F, "hip_ms": ms["hip"], "torch_ms": ms["torch"], "score": h["score"], "torch_score": t["score"],
            "samples_dev": float((h["samples"] - t["samples"]).abs().max()),
            "tiles_per_chunk": ops.H.lib().mmvae_cluster_sil_tiles_per_chunk(N, tiles, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_timing.txt"))
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cluster.py needs the MI355X"
    km = [bench_kmeans(D) for D in args.dims]
    sil = [bench_silhouette(F) for F in args.sizes]
    lines = [f"Latent cluster analysis, one MI355X (tools/bench_cluster.py): N = {N} rows, C = {C} clusters, float64, best of two "
             "warmed, alternated runs; device events around whole calls.  torch-ROCm composed = cdist / argmin / one-hot "
             "matmuls in float64 (k-means: all restarts until none changes, looked at every "
             f"{ops.KMEANS_CHECK_EVERY} iterations; silhouette: one unblocked 800 MB N x N temporary)", ""]
    for r in km:
        h, t = min(r["hip_ms"]), min(r["torch_ms"])
        lines.append(f"kmeans_fit, D {r['D']}, {R} restarts, iterations per restart {r['n_iter']}: HIP {h:.1f} ms  torch-ROCm "
                     f"composed {t:.1f} ms  HIP/torch {h / t:.2f}  (runs: HIP {[round(x, 1) for x in r['hip_ms']]}, torch "
                     f"{[round(x, 1) for x in r['torch_ms']]}; {r['labels_differ']} labels differ, torch counts "
                     f"{r['torch_n_iter']} iterations, inertia deviates {r['inertia_dev']:.1e} relative)")
    for r in sil:
        h, t = min(r["hip_ms"]), min(r["torch_ms"])
        lines.append(f"silhouette, F {r['F']} ({r['tiles_per_chunk']} column tiles per chunk at the most): HIP {h:.1f} ms  "
                     f"torch-ROCm composed {t:.1f} ms  HIP/torch {h / t:.2f}  (runs: HIP {[round(x, 1) for x in r['hip_ms']]}, "
                     f"torch {[round(x, 1) for x in r['torch_ms']]}; score {r['score']:.6f}, torch {r['torch_score']:.6f}, "
                     f"samples deviate {r['samples_dev']:.1e})")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps({"kmeans": km, "silhouette": sil}))


if __name__ == "__main__":
    main()
