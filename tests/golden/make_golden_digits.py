"""Generate the digit-classifier fixtures by running the REFERENCE's own modules (build container only).

    python tests/golden/make_golden_digits.py

Loads eval/mnistsvhn_helper.py of the reference (gensim / nltk / skimage, which it imports at the top and the classifiers
never touch, are stubbed here) and writes, as data only, digits/mnist.npz and digits/svhn.npz:

  w_<key>      the parameters of MNIST_Classifier / SVHN_Classifier after a seeded default init (weights x GAIN), rounded to fp16 and
               stored as fp16, so that both sides compute with identical values;
  images, labels   8 images (stored as fp16 values in [0, 1]; the MNIST ones with a zero border and every pixel below
               0.5 set to 0) and their digit labels;
  logp         the module's eval-mode output for them, computed with the module in .double();
  t_<key>      the parameters after 3 steps of CrossEntropyLoss + optim.Adam(lr=1e-3) on those 8 images with the module
               in .eval() (no dropout) and in .double(), stored as fp32;
  losses       the three losses.
"""
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("MMVAE_REFERENCE", "/root/reference/multimodal_compare")
OUT = os.path.join(HERE, "digits")


GAIN = 3.0      # applied to every weight tensor of the seeded default init


class _Permissive(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        obj = type(name, (), {})
        setattr(self, name, obj)
        return obj


def load_helper():
    for name in ("gensim", "gensim.models", "nltk", "nltk.tokenize", "skimage", "skimage.filters"):
        if name not in sys.modules:
            m = _Permissive(name)
            m.__path__ = []
            m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
            sys.modules[name] = m
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_mnistsvhn_helper",
                                                  os.path.join(REF_ROOT, "eval", "mnistsvhn_helper.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture(helper, kind, seed):
    torch.manual_seed(seed)
    net = (helper.MNIST_Classifier if kind == "mnist" else helper.SVHN_Classifier)()
    with torch.no_grad():
        # the default init gives log-probs that hardly move with the image (fc2's bias decides every argmax): a gain on
        # the weights makes the 8 images fall into several classes
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.mul_(GAIN)
        for p in net.parameters():
            p.copy_(p.half().float())
    out = {"w_" + k: v.detach().half().numpy() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    shape = (8, 1, 28, 28) if kind == "mnist" else (8, 3, 32, 32)
    x = torch.rand(*shape, generator=g)
    if kind == "mnist":
        x[..., :4, :] = 0
        x[..., -4:, :] = 0
        x[..., :, :4] = 0
        x[..., :, -4:] = 0
        x[x < 0.5] = 0
    x = x.half()
    y = torch.randint(0, 10, (8,), generator=g)
    out["images"], out["labels"] = x.numpy(), y.numpy().astype(np.int32)
    net.double().eval()
    xd = x.double()
    with torch.no_grad():
        logp = net(xd)
    assert logp.dtype == torch.float64 and logp.shape == (8, 10)
    out["logp"] = logp.numpy()
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.Adam(net.parameters(), lr=0.001)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = crit(net(xd).squeeze(), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert not net.training
    out.update({"t_" + k: v.detach().float().numpy() for k, v in net.state_dict().items()})
    out["losses"] = np.array(losses)
    np.savez(os.path.join(OUT, kind + ".npz"), **out)
    print(kind, "losses", losses, "pred", logp.argmax(-1).tolist())


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    h = load_helper()
    fixture(h, "mnist", 4321)
    fixture(h, "svhn", 8765)
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))
