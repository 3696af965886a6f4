"""Timing of the cross-modal retrieval of latents on the GPU box (no fallback: needs the MI355X).  Writes
profiles/retrieval_timing.txt (--out) and prints one JSON line.

ops.retrieval_ranks at N = 10 000 rows, S = 2 sets (both ordered pairs in one call), D = 32 and 64 (latent widths), every
metric, keep 0 and 10, on seeded sets (set 1 = set 0 permuted plus noise, as in tests/retrieval_reference.py) -- against the
same outputs composed from torch-ROCm ops in float64 on the same GPU, never an earlier run of this code.  Per pair, in blocks
of query rows (the N x N float64 matrix is 800 MB; a block of it is materialised):
  l2      |q|^2 + |g|^2 - 2 q @ g^T, clamped at 0 (the route of cdist's matmul mode)     w2   the same on [mean | scale] rows
  cosine  1 - (q @ g^T) / (|q| |g|^T)
  skl     broadcast differences (block, N, D): 1/2 [(vq + d^2) / vg + (vg + d^2) / vq] summed over D, minus D
  then gather of the partner's distance, two comparisons with row sums, topk(keep, largest=False).
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
N, S = 10000, 2
METRICS = ("l2", "cosine", "w2", "skl")


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
    loc, scale = np.empty((S, N, D), np.float32), np.empty((S, N, D), np.float32)
    loc[0], scale[0] = rs.standard_normal((N, D)), rs.uniform(0.1, 1.0, (N, D))
    match = rs.permutation(N).astype(np.int32)
    loc[1] = loc[0][match] + np.sqrt(2.0 * D) / 2.5 * rs.standard_normal((N, D))
    scale[1] = np.clip(scale[0][match] * np.exp2(rs.uniform(-1.0, 1.0, (N, D))), 0.1, 1.0)
    return loc, scale, match


# ---- the composed route, torch float64 on the GPU ---------------------------------------------------------------------------------
def torch_block(metric, ql, qs, gl, gs):
    if metric in ("l2", "w2"):
        if metric == "w2":
            ql, gl = torch.cat([ql, qs], 1), torch.cat([gl, gs], 1)
        return ((ql * ql).sum(1)[:, None] + (gl * gl).sum(1)[None, :] - 2.0 * (ql @ gl.t())).clamp_(min=0.0)
    if metric == "cosine":
        den = ql.norm(dim=1)[:, None] * gl.norm(dim=1)[None, :]
        return torch.where(den > 0, 1.0 - (ql @ gl.t()) / den, torch.ones_like(den))
    d2 = (ql[:, None, :] - gl[None, :, :]) ** 2
    vq, vg = (qs ** 2)[:, None, :], (gs ** 2)[None, :, :]
    return (0.5 * ((vq + d2) / vg + (vg + d2) / vq)).sum(2) - ql.shape[1]


def torch_ranks(loc, scale, match, metric, keep, block):
    loc64, scale64, m = loc.double(), scale.double(), match.long()
    out = {"d_match": [], "less": [], "equal": [], "nn_d": [], "nn_idx": []}
    for q, g in ops.retrieval_pairs(S):
        per = {k: [] for k in out}
        for i0 in range(0, N, block):
            rows = slice(i0, min(N, i0 + block))
            D = torch_block(metric, loc64[q, rows], scale64[q, rows], loc64[g], scale64[g])
            dm = D.gather(1, m[rows, None])
            per["d_match"].append(dm[:, 0])
            per["less"].append((D < dm).sum(1))
            per["equal"].append((D == dm).sum(1) - 1)
            if keep:
                top = D.topk(keep, dim=1, largest=False)
                per["nn_d"].append(top.values)
                per["nn_idx"].append(top.indices)
        for k in out:
            if per[k]:
                out[k].append(torch.cat(per[k]))
    return {k: torch.stack(v) for k, v in out.items() if v}


def alternate(hip, composed):
    ms = {"hip": [], "torch": []}
    for _ in range(2):
        t, out_t = timed(composed)
        ms["torch"].append(t)
        t, out_h = timed(hip)
        ms["hip"].append(t)
    return ms, out_h, out_t


def bench(D, metric, keep):
    loc, scale, match = (torch.from_numpy(a).to(DEV) for a in data(D, 1))
    block = 128 if metric == "skl" else 2048
    hip = lambda: ops.retrieval_ranks(loc, scale, match=match, metric=metric, keep=keep)      # noqa: E731
    composed = lambda: torch_ranks(loc, scale, match, metric, keep, block)                    # noqa: E731
    for _ in range(2):      # warm-up of every shape both sides use (first calls include code loading)
        hip()
        composed()
    ms, h, t = alternate(hip, composed)
    rank_h, rank_t = 1 + h["less"].long() + h["equal"].long(), 1 + t["less"] + t["equal"]
    r = {"D": D, "metric": metric, "keep": keep, "hip_ms": ms["hip"], "torch_ms": ms["torch"],
         "chunks": ops.H.lib().mmvae_retrieval_chunks(N, S * (S - 1)), "ranks_differ": int((rank_h != rank_t).sum()),
         "median_rank": float(rank_h.double().median()),
         "d_match_dev": float(((h["d_match"] - t["d_match"]).abs() / t["d_match"].abs().clamp(min=1e-300)).max())}
    if keep:
        r["neighbours_differ"] = int((h["nn_idx"].long() != t["nn_idx"]).sum())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_timing.txt"))
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--keeps", type=int, nargs="+", default=[0, 10])
    ap.add_argument("--metrics", nargs="+", default=list(METRICS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_retrieval.py needs the MI355X"
    res = [bench(D, metric, keep) for D in args.dims for metric in args.metrics for keep in args.keeps]
    lines = [f"Cross-modal retrieval of latents, one MI355X (tools/bench_retrieval.py): N = {N} rows, {S} sets, both ordered pairs "
             "in one call, float64, best of two warmed, alternated runs; device events around whole calls.  torch-ROCm composed "
             "= Gram matmuls (l2, cosine, w2) / broadcast differences (skl) in row blocks, comparisons, topk, in float64", ""]
    for r in res:
        h, t = min(r["hip_ms"]), min(r["torch_ms"])
        lines.append(f"{r['metric']:6s} D {r['D']:3d} keep {r['keep']:2d} ({r['chunks']} chunks): HIP {h:.2f} ms  torch-ROCm composed "
                     f"{t:.2f} ms  HIP/torch {h / t:.3f}  (runs: HIP {[round(x, 2) for x in r['hip_ms']]}, torch "
                     f"{[round(x, 2) for x in r['torch_ms']]}; median rank {r['median_rank']:.0f}, {r['ranks_differ']} of {2 * N} "
                     f"ranks differ, {r.get('neighbours_differ', 0)} neighbour slots differ, d_match deviates "
                     f"{r['d_match_dev']:.1e} relative)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps({"retrieval": res}))


if __name__ == "__main__":
    main()
