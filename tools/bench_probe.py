"""Timing of latent classification on the GPU box (no fallback: needs the MI355X).  Writes profiles/probe_timing.txt
(--out) and prints one JSON line.

(a) mmvae_probe_train for ONE epoch (one launch, all probes side by side) against the same epoch as nn.Linear +
    CrossEntropyLoss + optim.Adam on the same device, one probe after the other as the reference trains them; P = 1 and
    P = 15 at (N, D, C, batch) = (50000, 20, 10, 128) and (8192, 32, 10, 128).  Composition and kernel alternated, twice
    each; the kernel must not be slower than the composition by more than the composition's own run-to-run spread.
(b) a full classify_latents on cfg2 shapes (MoPoE, 3 subsets x 5 label columns = 15 probes, 30 epochs), with the share of
    the encoding and, for the encoding, latents_for (encoders + mixing) against forward() (the same + decoders).
    Reported, not gated.
Device events around whole calls that end in a synchronise; every shape warmed up first."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from multimodal_vae_comparison_amd import ops

DEV = "cuda"


def timed(fn, reps):
    """mean ms per call of `reps` back-to-back calls (device events, synchronised)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_epoch(P, N, D, C, batch, reps=3):
    g = torch.Generator().manual_seed(N + D + P)
    S = min(P, 3)
    A = (P + S - 1) // S
    centres = torch.randn(C, D, generator=g)
    labels = torch.randint(0, C, (A, N), generator=g)
    z = torch.stack([0.7 * centres[labels[0]] + torch.randn(N, D, generator=g) for _ in range(S)])
    zg, lg = z.to(DEV), labels.int().to(DEV)
    lg64 = labels.to(DEV)
    probes = [(p % S, p // S, C) for p in range(P)]
    state0 = ops.probe_state(P, D, C, DEV, seed=1)
    spe = (N + batch - 1) // batch
    state = state0.clone()

    def kern():
        state.copy_(state0)
        return ops.probe_train(state, zg, lg, probes, batch, 0, spe, validate=False)

    lins = [torch.nn.Linear(D, C).to(DEV) for _ in range(P)]
    opts = [torch.optim.Adam(lin.parameters(), lr=1e-3) for lin in lins]
    init = [ops.probe_weights(state0, p, C) for p in range(P)]
    ce = torch.nn.CrossEntropyLoss()

    def comp():
        last = []
        for p, (s, a, _) in enumerate(probes):
            with torch.no_grad():      # (the composition's counterpart of the kernel side's state.copy_)
                lins[p].weight.copy_(init[p][0])
                lins[p].bias.copy_(init[p][1])
            opt = opts[p]
            opt.state.clear()
            for i in range(0, N, batch):
                opt.zero_grad()
                loss = ce(lins[p](zg[s, i:i + batch]), lg64[a, i:i + batch])
                loss.backward()
                opt.step()
            last.append(loss.detach())
        return torch.stack(last)

    lk, lc = kern()[:, -1], comp()
    err = float((lk - lc).abs().max() / lc.abs().max())
    kern()
    t = {"comp": [], "kern": []}
    for _ in range(2):      # alternate: composition, kernel, composition, kernel
        t["comp"].append(timed(comp, 1))
        t["kern"].append(timed(kern, reps))
    spread = abs(t["comp"][0] - t["comp"][1])
    return {"P": P, "N": N, "D": D, "C": C, "batch": batch, "steps": spe, "kernel_ms": t["kern"],
            "composition_ms": t["comp"], "composition_spread_ms": spread, "last_step_loss_max_rel_diff": err,
            "ratio": max(t["kern"]) / min(t["comp"]), "ok": max(t["kern"]) <= min(t["comp"]) + spread}


def bench_classify(n_train=16, n_test=4, B=128, epochs=30):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import workload
    torch.manual_seed(0)
    _, cfg, dims, data, _ = workload("cfg2", B, device=DEV, seed=1)
    tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
    tr.model.eval()
    g = torch.Generator().manual_seed(2)
    n_classes = [3, 8, 2, 3, 2]      # CdSprites+: shape, colour, size, position, background
    mk = lambda n: [(data, torch.stack([torch.randint(0, c, (B,), generator=g) for c in n_classes], 1)) for _ in range(n)]
    train, test = mk(n_train), mk(n_test)
    run = lambda: tr.model.classify_latents(train, test, n_classes, epochs=epochs)
    given = tr.model.default_given()

    def encode():
        for g_ in given:
            for b, _ in train + test:
                tr.model.latents_for(b, g_)

    def encode_with_decoders():
        with torch.no_grad():
            for g_ in given:
                for b, _ in train + test:
                    tr.model.forward(tr.model._given_only(b, g_))

    out = run()
    encode()
    encode_with_decoders()
    res = {"config": "cfg2 mopoe", "N_train": n_train * B, "N_test": n_test * B, "D": tr.model.n_latents, "probes": len(out["probes"]),
           "epochs": epochs, "classify_ms": [timed(run, 1) for _ in range(2)],
           "encode_latents_for_ms": [timed(encode, 1) for _ in range(2)],
           "encode_forward_with_decoders_ms": [timed(encode_with_decoders, 1) for _ in range(2)]}
    return res


def report(res):
    L = ["Latent classification: timing (tools/bench_probe.py, one process, device events around synchronised calls,",
         "every shape warmed up, composition and kernel alternated: composition, kernel, composition, kernel)",
         f"box: one MI355X (gfx950; torch reports the device as \"{res['device']}\"), fp32", "",
         "(a) mmvae_probe_train, ONE epoch in one launch (all P probes side by side), vs the same epoch as nn.Linear +",
         "    CrossEntropyLoss + optim.Adam on the same device (the P probes one after the other), ms per epoch:",
         "    (P, N, D, C, batch)            steps  kernel            composition         spread    kernel/composition"]
    for r in res["epoch"]:
        L.append("    ({P}, {N}, {D}, {C}, {batch})".format(**r).ljust(35) + f"{r['steps']:<7d}"
                 + "{:.3f} {:.3f}".format(*r["kernel_ms"]).ljust(18) + "{:.1f} {:.1f}".format(*r["composition_ms"]).ljust(20)
                 + f"{r['composition_spread_ms']:.1f}".ljust(10) + f"{r['ratio']:.4f}")
    L.append("    requirement (kernel <= composition + its spread): " + ("met" if res["ok"] else "NOT met")
             + "; last-step loss, kernel vs composition: "
             + ", ".join(f"{r['last_step_loss_max_rel_diff']:.1e}" for r in res["epoch"]) + " relative.")
    c = res["classify"]
    L += ["", f"(b) full classify_latents, {c['config']}, {c['N_train']} train / {c['N_test']} test samples, D = {c['D']}, "
              f"{c['probes']} probes, {c['epochs']} epochs, ms:",
          "    classify_latents (encode both sets per subset + train + evaluate)   {:.1f} {:.1f}".format(*c["classify_ms"]),
          "    of which the encoding, latents_for (encoders + mixing only)          {:.1f} {:.1f}".format(*c["encode_latents_for_ms"]),
          "    the same encoding through forward() (encoders + mixing + decoders)   {:.1f} {:.1f}".format(*c["encode_forward_with_decoders_ms"]),
          "    reported, not gated.  latents_for skips the decoders: the difference of the last two lines is the decoders' share."]
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_probe needs the MI355X"
    shapes = [(P, N, D, C, b) for (N, D, C, b) in ((50000, 20, 10, 128), (8192, 32, 10, 128)) for P in (1, 15)]
    res = {"device": torch.cuda.get_device_name(0), "epoch": [bench_epoch(*s) for s in shapes], "classify": bench_classify()}
    res["ok"] = all(r["ok"] for r in res["epoch"])
    with open(args.out, "w") as f:
        f.write(report(res))
    print(json.dumps(res))
    sys.exit(0 if res["ok"] else 1)
