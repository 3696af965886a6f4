"""Restatement of the MNIST-SVHN digit classifiers and their training loop (eval/mnistsvhn_helper.py:191-226,
eval/eval_mnistsvhn.py:76-97) with torch.nn.functional on the CPU, in the dtype of the parameters it is given (float64 is
the yardstick of tests/test_digits_gpu.py; float32 measures how far plain fp32 drifts from it).  The dropout masks are
INPUTS (0 or 1/(1-p) floats, as ops.digit_masks re-materialises them); the loss is F.cross_entropy on the log-softmax
output, as the reference's CrossEntropyLoss is; the optimiser is torch.optim.Adam.  tests/golden/digits/*.npz pins this
file to the reference's own modules (tests/test_digits_host.py)."""
import torch
import torch.nn.functional as F

KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
INPUT = {"mnist": (1, 28, 28), "svhn": (3, 32, 32)}
FLAT = {"mnist": 320, "svhn": 500}


def shapes(kind):
    C = INPUT[kind][0]
    return {"conv1.weight": (10, C, 5, 5), "conv1.bias": (10,), "conv2.weight": (20, 10, 5, 5), "conv2.bias": (20,),
            "fc1.weight": (50, FLAT[kind]), "fc1.bias": (50,), "fc2.weight": (10, 50), "fc2.bias": (10,)}


def default_init(kind, seed):
    """nn.Conv2d / nn.Linear default init bounds (U(+-1/sqrt(fan_in))) from a generator -> {key: fp32 tensor}"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    sh = shapes(kind)
    for kw, kb in zip(KEYS[0::2], KEYS[1::2]):
        fan_in = 1
        for s in sh[kw][1:]:
            fan_in *= s
        bound = fan_in ** -0.5
        out[kw] = (torch.rand(*sh[kw], generator=g) * 2 - 1) * bound
        out[kb] = (torch.rand(*sh[kb], generator=g) * 2 - 1) * bound
    return out


def forward(kind, params, x, m2d=None, m1=None):
    """log-probabilities (N,10); m2d (N,20) / m1 (N,50) multiplicative masks or None (eval mode)"""
    dt = params["conv1.weight"].dtype
    x = x.to(dt)
    h = F.relu(F.max_pool2d(F.conv2d(x, params["conv1.weight"], params["conv1.bias"]), 2))
    c = F.conv2d(h, params["conv2.weight"], params["conv2.bias"])
    if m2d is not None:
        c = c * m2d.to(dt)[:, :, None, None]
    h = F.relu(F.max_pool2d(c, 2)).reshape(x.shape[0], FLAT[kind])
    h = F.relu(F.linear(h, params["fc1.weight"], params["fc1.bias"]))
    if m1 is not None:
        h = h * m1.to(dt)
    return F.log_softmax(F.linear(h, params["fc2.weight"], params["fc2.bias"]), dim=-1)


def grad(kind, params, x, y, m2d=None, m1=None, dtype=torch.float64):
    """-> ({key: gradient of the mean loss}, per-row loss (N,))"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    logp = forward(kind, p, x, m2d, m1)
    loss = F.cross_entropy(logp, y.long())
    loss.backward()
    return {k: v.grad for k, v in p.items()}, -logp.detach().gather(1, y.long()[:, None])[:, 0]


def train(kind, params, x, y, batch, epochs, lr=1e-3, m2d=None, m1=None, order=None, dtype=torch.float64):
    """`epochs` passes in minibatches of `batch` rows (the last one of a pass may be short); m2d (steps,batch,20) and
    m1 (steps,batch,50): the masks of every step by row position, or None.
    -> {"params", "exp_avg", "exp_avg_sq": {key: tensor}, "loss": (steps,) float64}"""
    p = {k: params[k].detach().to(dtype).clone().requires_grad_(True) for k in KEYS}
    opt = torch.optim.Adam([p[k] for k in KEYS], lr=lr)
    N, curve, t = x.shape[0], [], 0
    for e in range(epochs):
        idx = torch.arange(N) if order is None else order[e].long()
        for i in range(0, N, batch):
            rows = idx[i:i + batch]
            opt.zero_grad()
            logp = forward(kind, p, x[rows], None if m2d is None else m2d[t, :len(rows)],
                           None if m1 is None else m1[t, :len(rows)])
            loss = F.cross_entropy(logp, y[rows].long())
            loss.backward()
            opt.step()
            curve.append(float(loss.detach()))
            t += 1
    return {"params": {k: p[k].detach() for k in KEYS}, "exp_avg": {k: opt.state[p[k]]["exp_avg"] for k in KEYS},
            "exp_avg_sq": {k: opt.state[p[k]]["exp_avg_sq"] for k in KEYS},
            "loss": torch.tensor(curve, dtype=torch.float64)}


def prototypes(kind, proto_seed=7):
    """10 class prototypes (10,C,H,W): smooth blobs in [0,1]"""
    C, Hh, Ww = INPUT[kind]
    gp = torch.Generator().manual_seed(proto_seed + (0 if kind == "mnist" else 100))
    return F.interpolate(torch.rand(10, C, 7, 7, generator=gp), size=(Hh, Ww), mode="bilinear", align_corners=False)


def prototype_data(kind, N, seed, noise=0.25, proto_seed=7):
    """the class prototypes plus noise, clamped to [0,1] -> (x (N,C,H,W) fp32, y (N,) int64)"""
    C, Hh, Ww = INPUT[kind]
    proto = prototypes(kind, proto_seed)
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 10, (N,), generator=g)
    x = (proto[y] + noise * torch.randn(N, C, Hh, Ww, generator=g)).clamp_(0.0, 1.0)
    return x.contiguous(), y


def mnist_like(x):
    """a zero border of 4 pixels and every pixel below 0.5 set to 0: exact pool ties and dead ReLUs"""
    x = x.clone()
    x[..., :4, :] = 0
    x[..., -4:, :] = 0
    x[..., :, :4] = 0
    x[..., :, -4:] = 0
    x[x < 0.5] = 0
    return x


# ---- the dropout masks of csrc/digits.hip, restated on the host --------------------------------------------------------
_M = 0xFFFFFFFF


def _fmix(h):
    """murmur3 finaliser on numpy uint64 arrays holding 32-bit values (csrc/common.hpp: drop_fmix)"""
    import numpy as np
    h = np.asarray(h, dtype=np.uint64)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(_M)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(_M)
    return h ^ (h >> np.uint64(16))


def masks_host(kind, batch, step0, n_steps, seed=0, p=0.5):
    """(m2d (n_steps,batch,20), m1 (n_steps,batch,50)) fp32: element (t, r, u) is a function of (seed, kind, step0 + t, r, u)"""
    import numpy as np
    kind_id = {"mnist": 0, "svhn": 1}[kind]
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    out = []
    for site, units in ((0, 20), (1, 50)):
        m = np.ones((n_steps, batch * units), dtype=np.float32)
        if p > 0:
            for t in range(n_steps):
                step = step0 + t
                k = _fmix((seed & _M) ^ ((kind_id * 0x85EBCA77 + site * 0xC2B2AE3D + 0x27D4EB2F) & _M))
                k = _fmix((int(k) + (step & _M) * 0x9E3779B1) & _M)
                k = int(_fmix(int(k) ^ (step >> 32)))
                idx = np.arange(batch * units, dtype=np.uint64)
                h = _fmix((np.uint64(k) + (idx >> np.uint64(1)) * np.uint64(0x9E3779B1)) & np.uint64(_M))
                half = np.where(idx & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF))
                m[t] = np.where(half >= thr, inv_keep, 0.0)
        out.append(torch.from_numpy(m.reshape(n_steps, batch, units)))
    return out[0], out[1]
