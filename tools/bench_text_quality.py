"""Timing of the text generation quality on the GPU box (no fallback: needs the MI355X).  Writes
profiles/text_quality_timing.txt (--out) and prints one JSON line.

ops.text_quality at N = 10 000 pairs of the two text shapes of the shipped configs, T = 45 / V = 27 and T = 246 / V = 27, from fp32
logits, with the word level (sep = 0) and without, trim = 0, orders 1 .. 4, on seeded captions (words of 1 .. 8 letters, the
hypothesis a copy with a tenth of the letters replaced and, in every second row, one letter dropped) -- against
  (a) the parts torch-ROCm can express, in float64 on the same GPU: argmax, the position matches and cross_entropy (no edit
      distance, no LCS, no n-grams, no words: torch has no op for them);
  (b) the plain Python / numpy restatement of the tests (tests/text_quality_reference.py) on the first `--host-pairs` pairs on
      the host, scaled to N.
All sides warmed; a timed window is `--reps` calls between device events and ends in a synchronise; the median of `--rounds`
windows is reported.  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.nn.functional as F

from multimodal_vae_comparison_amd import ops

DEV = "cuda"
CONFIGS = ((45, 27), (246, 27))      # (T, V)


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def data(N, T, V, seed):
    """references (N, T) of words separated by single spaces (id 0) with their lengths, and logits whose argmax is a noisy copy"""
    g = torch.Generator().manual_seed(seed)
    letters = torch.randint(1, V, (N, T), generator=g)
    space = torch.rand(N, T, generator=g) < 0.2
    space[:, 0] = False
    space[:, 1:] &= ~space[:, :-1]
    ref = torch.where(space, torch.zeros_like(letters), letters)
    lens = torch.randint(T // 2, T + 1, (N,), generator=g)
    live = torch.arange(T)[None, :] < lens[:, None]
    ref = ref * live
    hyp = torch.where((torch.rand(N, T, generator=g) < 0.1) & live, torch.randint(0, V, (N, T), generator=g), ref)
    hyp[1::2, 3:-1] = hyp[1::2, 4:].clone()      # one letter dropped: the rest of the row shifts
    logits = torch.randn(N, T, V, generator=g)
    logits.scatter_add_(2, hyp[..., None], torch.full((N, T, 1), 6.0))
    return logits.to(DEV), ref.to(DEV), lens.to(DEV)


def torch_parts(x, ref, lens):
    """what torch-ROCm expresses of the outputs, in float64: pred, same, nll"""
    T = x.shape[1]
    live = torch.arange(T, device=x.device)[None, :] < lens[:, None]
    pred = x.argmax(-1)
    same = ((pred == ref) & live).sum(1)
    ce = F.cross_entropy(x.double().transpose(1, 2), ref, reduction="none")
    return {"pred": pred, "same": same, "nll": (ce * live).sum(1)}


def bench(N, T, V, reps, rounds, host_pairs):
    import text_quality_reference as R
    x, ref, lens = data(N, T, V, 1)
    sides = {"hip_words": lambda: ops.text_quality(x, ref, lens, trim=0, sep=0),
             "hip_tokens": lambda: ops.text_quality(x, ref, lens, trim=0),
             "torch": lambda: torch_parts(x, ref, lens)}
    for _ in range(2):      # warm-up of every shape every side uses (first calls include code loading)
        for fn in sides.values():
            fn()
    ms, out = {k: [] for k in sides}, {}
    for _ in range(rounds):
        for k, fn in sides.items():
            t, out[k] = timed(fn, reps)
            ms[k].append(t)
    t0 = time.perf_counter()
    host = R.text_quality(x[:host_pairs].cpu().numpy(), ref[:host_pairs].cpu().numpy(), lens[:host_pairs].cpu().numpy(), trim=0,
                          sep=0)
    host_ms = (time.perf_counter() - t0) * 1e3 * N / host_pairs
    h = out["hip_words"]
    agree = all(bool((h[lvl][k][:host_pairs].cpu() == torch.from_numpy(host[lvl][k])).all()) for lvl in ("token", "word")
                for k in host[lvl]) and bool((h["pred"][:host_pairs].cpu() == torch.from_numpy(host["pred"])).all())
    nll_bars = float(((h["nll"][:host_pairs].cpu() - torch.from_numpy(host["nll"])).abs() / torch.from_numpy(host["bar"])).max())
    same = bool((h["pred"] == out["torch"]["pred"]).all())
    return {"N": N, "T": T, "V": V, "ms": ms, "host_ms_scaled": host_ms, "host_pairs": host_pairs, "counts_equal_host": agree,
            "nll_vs_host_bars": nll_bars, "pred_equals_torch": same,
            "nll_vs_torch": float((h["nll"] - out["torch"]["nll"]).abs().max()),
            "lds_bytes": ops.H.lib().mmvae_text_quality_lds_bytes(T, T)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_quality_timing.txt"))
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_text_quality.py needs the MI355X"
    res = [bench(args.pairs, T, V, args.reps, args.rounds, args.host_pairs) for T, V in CONFIGS]
    lines = [f"Text generation quality, one MI355X (tools/bench_text_quality.py): N = {args.pairs} pairs from fp32 logits, trim 0, "
             f"orders 1 .. 4; median of {args.rounds} warmed rounds, device events around {args.reps} calls, each window ending in "
             "a synchronise.  torch-ROCm parts = argmax, position matches and float64 cross_entropy only (no alignment, no "
             f"n-grams, no words); host = the plain Python / numpy restatement on {args.host_pairs} pairs, scaled to N", ""]
    for r in res:
        m = {k: statistics.median(v) for k, v in r["ms"].items()}
        lines.append(f"text_quality, T = {r['T']}, V = {r['V']} ({r['lds_bytes']} B of LDS per one-wave workgroup): HIP with words "
                     f"{m['hip_words']:.3f} ms, tokens only {m['hip_tokens']:.3f} ms; torch-ROCm parts {m['torch']:.3f} ms "
                     f"(HIP with words / torch parts {m['hip_words'] / m['torch']:.2f}); host restatement {r['host_ms_scaled']:.0f} ms "
                     f"scaled (HIP with words / host {m['hip_words'] / r['host_ms_scaled']:.1e})  (rounds: words "
                     f"{[round(v, 3) for v in r['ms']['hip_words']]}, tokens {[round(v, 3) for v in r['ms']['hip_tokens']]}, torch "
                     f"{[round(v, 3) for v in r['ms']['torch']]}; counts equal to the host's: {r['counts_equal_host']}, nll within "
                     f"{r['nll_vs_host_bars']:.2g} bars of it, {r['nll_vs_torch']:.1e} from torch's; pred = torch's argmax: "
                     f"{r['pred_equals_torch']})")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps({"text_quality": res}))


if __name__ == "__main__":
    main()
