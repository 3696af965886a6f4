"""Timing of the MNIST-SVHN digit-coherence evaluation on the GPU box (no fallback: needs the MI355X).  Writes
profiles/digits_timing.txt (--out) and prints one JSON line.

(a) DigitClassifiers.fit: N = 60 000 synthetic images per network (10 prototypes + noise), batch 128, 1 epoch, both
    networks side by side on csrc/digits.hip -- against the reference's own way on the same GPU: the same two networks as
    torch nn.Modules (eval/mnistsvhn_helper.py's layers) under torch-ROCm eager with CrossEntropyLoss + optim.Adam, one
    after the other, the images already on the device.  HIP path and torch loop alternated, twice each; the torch loop is
    the baseline, never an earlier run of this code.
(b) digit_cross_coherence over N = 10 000 test pairs (batches of 250) and digit_joint_coherence at n = 1000, MoE on the
    MNIST-SVHN towers (D = 20), and the classifiers' forward alone (ops.digit_eval on 10 000 image pairs) against the two
    torch modules in eval mode.
Reported, not gated.  Device events around whole calls that end in a synchronise; every shape warmed up first."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn as nn
import torch.nn.functional as F

from multimodal_vae_comparison_amd import coherence as coh
from multimodal_vae_comparison_amd import ops

DEV = "cuda"
D = 20


class TorchDigitNet(nn.Module):
    """the baseline: the reference's classifier layers as an ordinary torch module"""

    def __init__(self, kind):
        super().__init__()
        C, self.flat = ops.DIGIT_INPUT[kind][0], (320 if kind == "mnist" else 500)
        self.conv1 = nn.Conv2d(C, 10, kernel_size=5)
        self.conv2 = nn.Conv2d(10, 20, kernel_size=5)
        self.conv2_drop = nn.Dropout2d()
        self.fc1 = nn.Linear(self.flat, 50)
        self.fc2 = nn.Linear(50, 10)

    def forward(self, x):
        x = F.relu(F.max_pool2d(self.conv1(x), 2))
        x = F.relu(F.max_pool2d(self.conv2_drop(self.conv2(x)), 2))
        x = F.relu(self.fc1(x.reshape(-1, self.flat)))
        x = F.dropout(x, training=self.training)
        return F.log_softmax(self.fc2(x), dim=-1)


def timed(fn, reps=1):
    """mean ms per call of `reps` back-to-back calls (device events, synchronised)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def data(kind, N, seed):
    C, Hh, Ww = ops.DIGIT_INPUT[kind]
    g = torch.Generator().manual_seed(seed)
    proto = F.interpolate(torch.rand(10, C, 7, 7, generator=g), size=(Hh, Ww), mode="bilinear", align_corners=False)
    y = torch.randint(0, 10, (N,), generator=g)
    return proto, y


def images(proto, y, seed, noise=0.5):
    g = torch.Generator().manual_seed(seed)
    return (proto[y] + noise * torch.randn(len(y), *proto.shape[1:], generator=g)).clamp_(0, 1)


def bench_fit(N, batch):
    pm, y = data("mnist", N, 1)
    ps, _ = data("svhn", N, 2)
    xm, xs = images(pm, y, 3).to(DEV), images(ps, y, 4).to(DEV)
    yd = y.to(DEV)
    chunk = 2000
    train = [({"mod_1": {"data": xm[i:i + chunk], "masks": None}, "mod_2": {"data": xs[i:i + chunk], "masks": None}},
              y[i:i + chunk]) for i in range(0, N, chunk)]
    test = train[:5]

    def hip_fit():
        torch.manual_seed(0)
        cls = coh.DigitClassifiers().to(DEV)
        curve = cls.fit(train, 1, batch_size=batch, lr=1e-3, seed=0, p=0.5)
        return cls, curve

    def torch_fit(n=N):
        torch.manual_seed(0)
        nets = {"mnist": TorchDigitNet("mnist").to(DEV), "svhn": TorchDigitNet("svhn").to(DEV)}
        last = {}
        for k, x in (("mnist", xm), ("svhn", xs)):
            net = nets[k].train()
            crit, opt = nn.CrossEntropyLoss(), torch.optim.Adam(net.parameters(), lr=1e-3)
            for i in range(0, n, batch):
                opt.zero_grad()
                loss = crit(net(x[i:min(i + batch, n)]), yd[i:min(i + batch, n)])
                loss.backward()
                opt.step()
            last[k] = loss
        return nets, last

    # warm-up of both at a short length that ends on the epoch's tail shape (N % batch rows), then alternate
    n_warm = min(N, 4 * batch + N % batch)
    short = [({m: {"data": v["data"][:n_warm], "masks": None} for m, v in train[0][0].items()}, train[0][1][:n_warm])]
    coh.DigitClassifiers().to(DEV).fit(short, 1, batch_size=batch)
    torch_fit(n_warm)
    t_hip, t_torch = [], []
    cls = nets = None
    for _ in range(2):
        holder = {}
        t_torch.append(timed(lambda: holder.update(t=torch_fit())))
        nets = holder["t"][0]
        t_hip.append(timed(lambda: holder.update(h=hip_fit())))
        cls, curve = holder["h"]
    steps = (N + batch - 1) // batch
    acc = cls.accuracy(test)
    with torch.no_grad():
        acc_t = {k: float((nets[k].eval()(x[:5 * chunk]).argmax(-1) == yd[:5 * chunk]).float().mean())
                 for k, x in (("mnist", xm), ("svhn", xs))}
    return {"N": N, "batch": batch, "steps": steps, "hip_ms": t_hip, "torch_ms": t_torch,
            "ratio_hip_over_torch": min(t_hip) / min(t_torch), "launches_per_step": 2,
            "hip_train_accuracy": acc, "torch_train_accuracy": acc_t,
            "hip_loss_first_last": [[float(c[0]), float(c[-1])] for c in curve]}


def bench_eval(N, reps):
    from multimodal_vae_comparison_amd.models.trainer import MultimodalVAE
    from multimodal_vae_comparison_amd.synthetic import MS_MODS, config_from_mods, mnist_svhn_batch
    torch.manual_seed(0)
    cfg, dims = config_from_mods("moe", MS_MODS, D, batch_size=250)
    tr = MultimodalVAE(cfg, feature_dims=dims, device=DEV)
    tr.model.eval()
    cls = coh.DigitClassifiers().to(DEV)
    g = torch.Generator().manual_seed(5)
    batches = [(mnist_svhn_batch(250, seed=3 + i, device=DEV), torch.randint(0, 10, (250,), generator=g))
               for i in range(0, N, 250)]
    xm = torch.cat([b["mod_1"]["data"] for b, _ in batches]).contiguous()
    xs = torch.cat([b["mod_2"]["data"] for b, _ in batches]).contiguous()
    nets = [TorchDigitNet("mnist").to(DEV).eval(), TorchDigitNet("svhn").to(DEV).eval()]

    def torch_pred():
        with torch.no_grad():
            return nets[0](xm).argmax(-1), nets[1](xs).argmax(-1)

    cross = lambda: tr.model.digit_cross_coherence(batches, cls)
    joint = lambda: tr.model.digit_joint_coherence(cls, n=1000)
    pred = lambda: cls.predict(xm, xs)
    cross(), joint(), pred(), torch_pred()
    return {"N": N, "cross_ms": [timed(cross, reps) for _ in range(2)], "joint_ms": [timed(joint, reps) for _ in range(2)],
            "predict_hip_ms": [timed(pred, reps) for _ in range(2)], "predict_torch_ms": [timed(torch_pred, reps) for _ in range(2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "digits_timing.txt"))
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_digits.py needs the MI355X"
    res = {"fit": bench_fit(args.n, args.batch), "eval": bench_eval(10000, args.reps)}
    f_, e = res["fit"], res["eval"]
    lines = ["MNIST-SVHN digit coherence, one MI355X (tools/bench_digits.py)", "",
             f"fit, both classifiers, N {f_['N']} batch {f_['batch']} 1 epoch ({f_['steps']} steps, {f_['launches_per_step']} "
             f"launches per step for both networks): HIP {min(f_['hip_ms']):.1f} ms  torch-ROCm eager + optim.Adam "
             f"{min(f_['torch_ms']):.1f} ms  HIP/torch {f_['ratio_hip_over_torch']:.3f}  (runs: HIP {f_['hip_ms']}, torch "
             f"{f_['torch_ms']})",
             f"  accuracy on the first 10 000 train images after the epoch: HIP {f_['hip_train_accuracy']}, torch "
             f"{f_['torch_train_accuracy']}; HIP loss first / last step {f_['hip_loss_first_last']}",
             f"digit_cross_coherence N {e['N']} (batches of 250), MoE D {D}: {min(e['cross_ms']):.2f} ms  (runs: {e['cross_ms']})",
             f"digit_joint_coherence n 1000: {min(e['joint_ms']):.2f} ms  (runs: {e['joint_ms']})",
             f"both classifiers' forward on {e['N']} image pairs: HIP {min(e['predict_hip_ms']):.3f} ms  torch eager "
             f"{min(e['predict_torch_ms']):.3f} ms  (runs: HIP {e['predict_hip_ms']}, torch {e['predict_torch_ms']})"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
