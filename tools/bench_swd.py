"""Timing of the sliced Wasserstein / marginal KS statistics on the GPU box (no fallback: needs the MI355X).  Writes
profiles/swd_timing.txt (--out) and prints one JSON line.

Seeded Gaussian rows (the second set 0.7 N(0, 1) + 0.3): latents (n = 1000 and 8192, F = 32 and 64, L = 128 drawn directions,
n_y = n_x and n_y = n_x - 1), pixels (n = 1000, F = 12288, L = 128) and axis mode.  ops.swd_slices -- the finite check and
all four launches, the directions already on the device -- against the same outputs composed from torch-ROCm float64 ops on
the same GPU, never an earlier run of this code: one matmul per set, torch.sort, |x_(i) - y_(i)| for equal sizes and the gather
over the breakpoints of the grid of 1 / (n_x n_y) for unequal ones, and two batched torch.searchsorted for the KS counts.
Both sides warmed, alternated, three times each; device events around whole calls that end in a synchronise.  Reported with
the largest relative deviation of w and whether ks agrees; reported, not gated."""
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
SEED, RUNS = 0, 3
# (what, n_x, n_y, F, L; L None: axis mode)
SHAPES = [("latents", n, n - less, F, 128) for n in (1000, 8192) for F in (32, 64) for less in (0, 1)] + \
         [("pixels", 1000, 1000, 12288, 128), ("axis", 1000, 1000, 64, None), ("axis", 8192, 8191, 64, None),
          ("axis", 1000, 1000, 1024, None)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def torch_slices(X, Y, dirs):
    """the composed route: (w (L, 2) float64, ks (L,) int64)"""
    n_x, n_y = X.shape[0], Y.shape[0]
    if dirs is None:
        px, py = X.double().T.contiguous(), Y.double().T.contiguous()
    else:
        px, py = dirs @ X.double().T, dirs @ Y.double().T
    xs, ys = torch.sort(px, dim=1).values, torch.sort(py, dim=1).values
    if n_x == n_y:
        d = (xs - ys).abs()
        w = torch.stack([d.mean(1), (d * d).mean(1)], 1)
    else:
        cuts = torch.unique(torch.cat([torch.arange(n_x + 1, device=X.device) * n_y, torch.arange(n_y + 1, device=X.device) * n_x]))
        length = (cuts[1:] - cuts[:-1]).double()
        d = (xs[:, cuts[:-1] // n_y] - ys[:, cuts[:-1] // n_x]).abs()
        w = torch.stack([(d * length).sum(1), (d * d * length).sum(1)], 1) / float(n_x * n_y)
    pooled = torch.cat([xs, ys], 1)
    cx, cy = torch.searchsorted(xs, pooled, right=True), torch.searchsorted(ys, pooled, right=True)
    return w, (n_y * cx - n_x * cy).abs().amax(1)


def bench(what, n_x, n_y, F, L):
    rs = np.random.RandomState(11)
    X = torch.from_numpy(rs.standard_normal((n_x, F)).astype(np.float32)).to(DEV)
    Y = torch.from_numpy((0.7 * rs.standard_normal((n_y, F)) + 0.3).astype(np.float32)).to(DEV)
    dirs = None if L is None else torch.from_numpy(ops.swd_draw(F, L, SEED)).to(DEV)
    hip = lambda: ops.swd_slices(X, Y, dirs)      # noqa: E731
    composed = lambda: torch_slices(X, Y, dirs)      # noqa: E731
    for _ in range(2):      # warm-up of every shape both sides use (first calls include code loading)
        hip()
        composed()
    res = {"what": what, "n_x": n_x, "n_y": n_y, "F": F, "L": F if L is None else L, "hip_ms": [], "torch_ms": []}
    for _ in range(RUNS):
        t, out_t = timed(composed)
        res["torch_ms"].append(t)
        t, out_h = timed(hip)
        res["hip_ms"].append(t)
    res["w_dev"] = float(((out_h[0] - out_t[0]).abs() / out_t[0].abs()).max())
    res["ks_equal"] = bool(torch.equal(out_h[1], out_t[1]))
    res["swd2"] = float(out_h[0][:, 1].mean().sqrt())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swd_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_swd.py needs the MI355X"
    res = []
    for shape in SHAPES:
        res.append(bench(*shape))
        print(f"{shape} done", file=sys.stderr, flush=True)
    lines = ["Sliced Wasserstein and marginal KS statistics per direction (W_1, W_2^2, the KS numerator), one MI355X "
             f"(tools/bench_swd.py): float64, best of {RUNS} warmed, alternated runs; device events around whole calls.  HIP = "
             "ops.swd_slices (the finite check, the projection on the fp64 MFMA, two sorts, one merge walk); torch-ROCm composed "
             "= matmul, torch.sort, the gather over the grid's breakpoints (unequal sizes), two batched searchsorted", ""]
    for r in res:
        h, t = min(r["hip_ms"]), min(r["torch_ms"])
        lines.append(f"{r['what']}: n_x {r['n_x']}, n_y {r['n_y']}, F {r['F']}, L {r['L']}:")
        lines.append(f"  HIP {h:.2f} ms  torch-ROCm composed {t:.2f} ms  HIP/torch {h / t:.2f}  (runs: HIP "
                     f"{[round(x, 2) for x in r['hip_ms']]}, torch {[round(x, 2) for x in r['torch_ms']]})")
        lines.append(f"  w deviates {r['w_dev']:.1e} relative at the most, ks {'equal' if r['ks_equal'] else 'DIFFERS'}; swd2 "
                     f"{r['swd2']:.6g}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
