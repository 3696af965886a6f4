"""Timing of the exact t-SNE embedding of the latent analysis on the GPU box (no fallback: needs the MI355X).  Writes
profiles/tsne_timing.txt (--out) and prints one JSON line.

ops.tsne_embed at N = 500 (the reference's 2 x 250 samples), 2 000 and 10 000 points of D = 32 clustered dimensions, a
fixed 1000 iterations (stopping disabled), the objective logged every 50th iteration -- against the same algorithm
composed from torch-ROCm ops on the same GPU (torch.cdist, elementwise ops, sum, one matmul for the weighted sum of the
y_j), on the same P, the objective also every 50th iteration.  The torch loop is the baseline, never an earlier run of this
code.  Both warmed, alternated, twice each; device events around whole calls that end in a synchronise.  Also: the
iterations alone (ops.tsne_run in calls of 50), with the objective every 50th iteration and in every iteration, and at
N = 10 000 the share of the HBM peak that the P stream (4 N^2 bytes per iteration) reaches.  Reported, not gated."""
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
D = 32
ITERS = 1000
HBM_PEAK = 8.0e12      # bytes / s, the MI355X's specified HBM3E rate
EPS = 2.220446049250313e-16


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def data(N, seed=0):
    rs = np.random.RandomState(seed)
    centres = 3.0 * rs.standard_normal((10, D))
    return torch.from_numpy((centres[np.arange(N) % 10] + rs.standard_normal((N, D))).astype(np.float32)).to(DEV)


def torch_iterations(P, Y0, lr, iters, kl_every=50):
    """the baseline: the iteration of include/mmvae_hip.h as a torch user would compose it"""
    Y, upd, gains = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
    kls = []
    for it in range(iters):
        ex, mom = (12.0, 0.5) if it < 250 else (1.0, 0.8)
        w = 1.0 / (1.0 + torch.cdist(Y, Y).square_())
        w.fill_diagonal_(0.0)
        Q = w / w.sum(dtype=torch.float64).float()
        eP = ex * P
        M = (eP - Q) * w
        g = 4.0 * (M.sum(1, keepdim=True) * Y - M @ Y)
        if (it + 1) % kl_every == 0:
            off = Q > 0
            kls.append(torch.where(off, eP * torch.log(eP.clamp_min(EPS) / Q.clamp_min(1e-37)), 0.0).sum(dtype=torch.float64))
        gains = torch.where(upd * g < 0, gains + 0.2, gains * 0.8).clamp_min_(0.01)
        upd = mom * upd - lr * gains * g
        Y = Y + upd
        if (it + 1) % 50 == 0:
            float(kls[-1])      # (the look at the objective that the stopping rule takes: one synchronisation)
    return Y, float(kls[-1])


def hip_iterations(P, Y0, lr, iters, kl_every):
    state = ops.tsne_state(Y0)
    for it in range(0, iters, 50):
        log = ops.tsne_run(state, P, it, 50, lr, kl_every=kl_every)
        float(log[-1, 1])
    return state[0], float(log[-1, 0])


def bench(N, perplexity=30.0):
    X = data(N)
    lr = ops.tsne_default_lr(N)
    Y0 = ops.tsne_default_init(N).to(DEV)
    embed = lambda: ops.tsne_embed(X, perplexity=perplexity, max_iter=ITERS, n_iter_without_progress=10 ** 6, min_grad_norm=0.0)
    t_p, (P, _) = timed(lambda: ops.tsne_joint_probabilities(X, perplexity))      # (first call: includes code loading)
    t_p, (P, _) = timed(lambda: ops.tsne_joint_probabilities(X, perplexity))
    Pc = P.contiguous()
    # warm-up of every shape both sides use
    ops.tsne_embed(X, perplexity=perplexity, max_iter=250, n_iter_without_progress=10 ** 6, min_grad_norm=0.0)
    torch_iterations(Pc, Y0, lr, 50)
    hip_iterations(P, Y0, lr, 50, 1)
    res = {"N": N, "P_ms": t_p, "embed_ms": [], "hip_iter_ms": [], "torch_iter_ms": []}
    for _ in range(2):
        t, (Yt, kl_t) = timed(lambda: torch_iterations(Pc, Y0, lr, ITERS))
        res["torch_iter_ms"].append(t)
        t, (Yh, kl_h) = timed(lambda: hip_iterations(P, Y0, lr, ITERS, 50))
        res["hip_iter_ms"].append(t)
        t, out = timed(embed)
        res["embed_ms"].append(t)
    res["hip_iter_kl_every_1_ms"] = timed(lambda: hip_iterations(P, Y0, lr, ITERS, 1))[0]
    res["kl_hip"], res["kl_torch"], res["kl_embed"] = kl_h, kl_t, out["kl_divergence"]
    res["us_per_iteration_hip"] = 1e3 * min(res["hip_iter_ms"]) / ITERS
    res["us_per_iteration_torch"] = 1e3 * min(res["torch_iter_ms"]) / ITERS
    res["ratio_hip_over_torch"] = min(res["hip_iter_ms"]) / min(res["torch_iter_ms"])
    res["p_stream_share_of_hbm_peak"] = 4.0 * N * N / (1e-6 * res["us_per_iteration_hip"]) / HBM_PEAK
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_timing.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000, 10000])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsne.py needs the MI355X"
    res = [bench(N) for N in args.sizes]
    lines = ["Exact t-SNE of the latent analysis, one MI355X (tools/bench_tsne.py): D 32, perplexity 30, 1000 iterations, "
             "stopping disabled, objective every 50th iteration", ""]
    for r in res:
        lines += [f"N {r['N']}: tsne_embed {min(r['embed_ms']):.1f} ms (joint P {r['P_ms']:.2f} ms of it; runs {r['embed_ms']})",
                  f"  1000 iterations alone: HIP {min(r['hip_iter_ms']):.1f} ms = {r['us_per_iteration_hip']:.1f} us per "
                  f"iteration (2 launches)  torch-ROCm composed {min(r['torch_iter_ms']):.1f} ms = "
                  f"{r['us_per_iteration_torch']:.1f} us per iteration  HIP/torch {r['ratio_hip_over_torch']:.3f}  (runs: HIP "
                  f"{r['hip_iter_ms']}, torch {r['torch_iter_ms']})",
                  f"  objective in every iteration instead of every 50th: HIP {r['hip_iter_kl_every_1_ms']:.1f} ms",
                  f"  P stream 4 N^2 bytes per iteration: {100 * r['p_stream_share_of_hbm_peak']:.1f} % of the 8 TB/s HBM peak"
                  f"{' (P fits the 256 MiB Infinity Cache: not an HBM figure)' if 4 * r['N'] ** 2 <= 256 * 2 ** 20 else ''}",
                  f"  final objective: HIP {r['kl_embed']:.4f} (exaggeration off), at the last check HIP {r['kl_hip']:.4f} "
                  f"torch {r['kl_torch']:.4f}"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
