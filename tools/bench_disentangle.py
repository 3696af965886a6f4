"""Timing of the aggregate posterior behind the disentanglement metrics on the GPU box (no fallback: needs the MI355X).
Writes profiles/disentangle_timing.txt (--out) and prints one JSON line.

N = 500 / 2 000 / 10 000 samples, D = 16 / 32 / 64 latent dimensions, K = 0 and 5 label rows of 4 classes, Normal and
Laplace posteriors (the seeded generator of tests/disentangle_reference.py, restated).  Timed is the whole
ops.aggregate_posterior call (validation, workspace, the four launches, the finite check of the result) and, apart, the
four launches alone through the C entry point on preallocated buffers -- against one baseline, never an earlier run of this
code: the same three outputs composed from torch-ROCm float64 ops on the same GPU, walked in blocks of sample rows whose
(rows, N, D) float64 temporary stays below 2^27 elements (1 GB), torch.logsumexp (a running maximum) for every sum, one
masked pass per label row.  Both sides warmed, alternated, twice each; device events around windows of whole calls that
end in a synchronise, the calls repeated until a window lasts 50 ms or so.  Reported with the launches' exp / s: N^2 (D + 1)
exps, one per (n, m, d) and one per (n, m), over the launches' time.  Reported, not gated."""
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
CLASSES = 4
BLOCK_ELEMENTS = 1 << 27
WINDOW_MS = 50.0


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def data(N, D, K, laplace, seed=3):
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, CLASSES, size=(K, N)).astype(np.int32) if K > 0 else None
    loc = 0.4 * rng.standard_normal((N, D))
    for k in range(min(K, D)):
        loc[:, k] += 1.5 * (labels[k] - 0.5 * (CLASSES - 1))
    if 0 < K < D:
        loc[:, K] += 0.7 * (labels[0] - 0.5 * (CLASSES - 1))
    scale = np.exp(rng.uniform(np.log(0.25), np.log(1.2), size=(N, D)))
    e = rng.laplace(size=(N, D)) if laplace else rng.standard_normal((N, D))
    loc, scale = loc.astype(np.float32), scale.astype(np.float32)
    z = (loc.astype(np.float64) + scale.astype(np.float64) * e).astype(np.float32)
    return tuple(None if a is None else torch.from_numpy(a).to(DEV) for a in (z, loc, scale, labels))


# ---- the composed route, torch float64 on the GPU, in blocks of sample rows ---------------------------------------------------
def torch_aggregate(z, loc, scale, laplace, labels):
    N, D = z.shape
    z, loc, s = z.double(), loc.double(), scale.double()
    c = torch.log(2.0 * s) if laplace else torch.log(s) + 0.5 * math.log(2.0 * math.pi)
    K = 0 if labels is None else labels.shape[0]
    joint = torch.empty(N, dtype=torch.float64, device=z.device)
    marginal = torch.empty(N, D, dtype=torch.float64, device=z.device)
    cond = torch.empty(K, N, D, dtype=torch.float64, device=z.device) if K else None
    step = max(1, BLOCK_ELEMENTS // (N * D))
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        t = (z[lo:hi, None, :] - loc[None]) / s[None]
        l = (-t.abs() if laplace else -0.5 * t * t) - c[None]
        del t
        joint[lo:hi] = torch.logsumexp(l.sum(2), 1) - math.log(N)
        marginal[lo:hi] = torch.logsumexp(l, 1) - math.log(N)
        for k in range(K):
            same = labels[k, lo:hi, None] == labels[k][None, :]
            cond[k, lo:hi] = torch.logsumexp(l.masked_fill(~same[:, :, None], float("-inf")), 1) \
                - same.sum(1).double().log()[:, None]
    return {"joint": joint, "marginal": marginal, "conditional": cond}


def bench(N, D, K, laplace):
    z, loc, scale, labels = data(N, D, K, laplace)
    L, H = ops.H.lib(), ops.H
    chunks = L.mmvae_aggpost_chunks(N, D)
    ws = torch.empty(L.mmvae_aggpost_ws_doubles(N, D, K, 0), dtype=torch.float64, device=DEV)
    joint = torch.empty(N, dtype=torch.float64, device=DEV)
    marginal = torch.empty(N, D, dtype=torch.float64, device=DEV)
    cond = torch.empty(max(K, 1), N, D, dtype=torch.float64, device=DEV)

    def launches():
        H.check(L.mmvae_aggpost_lse(H.ptr(z), H.ptr(loc), H.ptr(scale), int(laplace), H.ptr(labels), H.ptr(ws), H.ptr(joint),
                                    H.ptr(marginal), H.ptr(cond), N, D, K, 0, H.stream()), "mmvae_aggpost_lse")

    sides = {"op": lambda: ops.aggregate_posterior(z, loc, scale, laplace=laplace, labels=labels), "launches": launches,
             "torch": lambda: torch_aggregate(z, loc, scale, laplace, labels)}
    reps = {}
    for name, fn in sides.items():      # warm-up of every shape (first calls include code loading), then the window's length
        fn()
        t, _ = timed(fn)
        reps[name] = max(1, min(200, int(WINDOW_MS / max(t, 1e-3))))
    res = {"N": N, "D": D, "K": K, "laplace": laplace, "chunks": chunks, "reps": reps,
           "op_ms": [], "launches_ms": [], "torch_ms": []}
    for _ in range(2):
        for name, fn in sides.items():
            t, out = timed(fn, reps[name])
            res[f"{name}_ms"].append(t)
            if name == "op":
                got = out
            elif name == "torch":
                ref = out
    res["dev"] = max(float((got[p] - ref[p]).abs().max()) for p in ("joint", "marginal", "conditional") if ref[p] is not None)
    res["exp_per_s"] = N * N * (D + 1) / (1e-3 * min(res["launches_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disentangle_timing.txt"))
    ap.add_argument("--rows", type=int, nargs="+", default=[500, 2000, 10000])
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--factors", type=int, nargs="+", default=[0, 5])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_disentangle.py needs the MI355X"
    res = []
    for laplace in (False, True):
        for N in args.rows:
            for D in args.dims:
                for K in args.factors:
                    res.append(bench(N, D, K, laplace))
                    print(f"{'Laplace' if laplace else 'Normal'} N {N} D {D} K {K} done", file=sys.stderr, flush=True)
    lines = ["Aggregate posterior (joint, marginal and class-conditional log-densities), one MI355X (tools/bench_disentangle.py): "
             "float64 outputs, best of two warmed, alternated windows of whole calls (device events; calls repeated until a "
             "window lasts about 50 ms).  op = ops.aggregate_posterior (validation, workspace, four launches, finite check); "
             "launches = the four launches alone on preallocated buffers; torch = the same outputs composed from torch-ROCm "
             "float64 ops in row blocks of at most 2^27 elements, torch.logsumexp, one masked pass per label row.  exp/s = "
             "N^2 (D + 1) exps over the launches' time (the fp64 vector peak is 39.3 T fused multiply-adds per second; a "
             "double-precision exp is some tens of them).  K label rows of 4 classes.", ""]
    lines.append(f"{'family':8s} {'N':>6s} {'D':>3s} {'K':>2s} {'chunks':>6s} {'op ms':>9s} {'launches ms':>12s} {'torch ms':>10s} "
                 f"{'op/torch':>9s} {'launches/torch':>15s} {'G exp/s':>8s} {'max |HIP - torch|':>18s}")
    for r in res:
        o, k, t = min(r["op_ms"]), min(r["launches_ms"]), min(r["torch_ms"])
        lines.append(f"{'Laplace' if r['laplace'] else 'Normal':8s} {r['N']:6d} {r['D']:3d} {r['K']:2d} {r['chunks']:6d} {o:9.3f} "
                     f"{k:12.3f} {t:10.3f} {o / t:9.3f} {k / t:15.3f} {1e-9 * r['exp_per_s']:8.1f} {r['dev']:18.2e}")
    lines += ["", "runs (ms per call; op | launches | torch):"]
    for r in res:
        lines.append(f"  {'Laplace' if r['laplace'] else 'Normal'} N {r['N']} D {r['D']} K {r['K']}: "
                     + " | ".join(str([round(x, 3) for x in r[f'{n}_ms']]) + f" x{r['reps'][n]}" for n in ("op", "launches", "torch")))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
