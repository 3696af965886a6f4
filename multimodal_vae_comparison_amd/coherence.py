"""Generation coherence of the CdSprites+ benchmark (reference: eval/eval_cdsprites.py, eval/train_classifiers.py).

Three parts:
  * the caption semantics, restated on token ids / strings on the host (which attribute value a caption names, which
    one a decoded caption spells at the word position its level prescribes, the letter count);
  * AttributeClassifier / AttributeClassifiers: the reference's image classifiers (one CNN per attribute) on the
    k4-s2 conv kernels, their heads in one ops.cls_head launch;
  * the scoring helpers TorchMMVAE.cross_coherence / joint_coherence (models/evaluation.py) are built from.
For the MNIST-SVHN benchmark (reference: eval/eval_mnistsvhn.py) DigitClassifier / DigitClassifiers at the end of the file:
the two LeNet-style digit classifiers, trained and scored on csrc/digits.hip (TorchMMVAE.digit_cross_coherence /
digit_joint_coherence).  For the cross-modal correlation (reference: eval/mnistsvhn_helper.py) sif_weights and
SentenceFeatures after them: the frequency-weighted caption feature (TorchMMVAE.cross_modal_correlation).  Nothing here
imports the models: they import this module.
"""
import torch
import torch.nn as nn

from . import hipops as H
from . import ops

ALPHABET = " abcdefghijklmnopqrstuvwxyz"

# attributes a caption of each level names, in caption order
LEVEL_ATTRIBUTES = {1: ("shape",), 2: ("size", "shape"), 3: ("size", "color", "shape"),
                    4: ("size", "color", "shape", "position"),
                    5: ("size", "color", "shape", "position", "background")}
# the values a caption is searched for, in search order (the first one found wins: "white" before "red", ...)
SEARCH_ORDER = {"shape": ("heart", "ellipse", "square"),
                "size": ("small", "big"),
                "color": ("white", "red", "yellow", "green", "blue", "pink"),
                "background": ("on light", "on dark"),
                "position": ("at top left", "at top right", "at bottom right", "at bottom left")}
# class index -> value of the image classifiers (the order they were trained with)
CLASS_NAMES = {"shape": ("square", "ellipse", "heart"),
               "size": ("big", "small"),
               "color": ("blue", "green", "red", "yellow", "pink"),
               "position": ("at top left", "at top right", "at bottom left", "at bottom right"),
               "background": ("on light", "on dark")}
# where a decoded caption is read for an attribute: one word index per level, or a run of words joined by spaces
_WORD_OF = {"size": {1: 0, 2: 0, 3: 0, 4: 0, 5: 0}, "shape": {1: 0, 2: 1, 3: 2, 4: 2, 5: 2}, "color": {3: 1, 4: 1, 5: 1}}
_WORDS_OF = {"background": (-2, -1), "position": (3, 4, 5, 6)}
UNKNOWN = "Unknown"


def _level_attributes(level):
    if level not in LEVEL_ATTRIBUTES:
        raise ValueError(f"coherence: level {level!r} (the CdSprites+ levels are 1 .. 5)")
    return LEVEL_ATTRIBUTES[level]


def ids_to_text(ids, length=None):
    """token ids -> string over ALPHABET (id 0 is the space); `length`: keep the first `length` symbols"""
    ids = [int(i) for i in ids]
    if length is not None:
        ids = ids[:max(int(length), 0)]
    return "".join(ALPHABET[i] for i in ids)


def text_to_ids(text, T=None):
    """string -> ids (a symbol outside ALPHABET becomes 0, as an all-zero one-hot row decodes), padded with 0 to T"""
    ids = [max(ALPHABET.find(ch), 0) for ch in text.lower()]
    if T is not None:
        ids = (ids + [0] * T)[:T]
    return ids


def _first_contained(values, text):
    """the first of `values` (in their order) that occurs in `text` as a SUBSTRING, lower-cased; None if none does"""
    text = text.lower()
    for v in values:
        if v.lower() in text:
            return v.lower()
    return None


def attribute_in_caption(attribute, caption):
    """the value of `attribute` a ground-truth caption names: a substring search over the whole caption"""
    return _first_contained(SEARCH_ORDER[attribute], caption)


def attribute_in_decoded(attribute, text, level):
    """the value of `attribute` a DECODED caption spells at the place its level prescribes: size = word 0, color = word 1,
    shape = word 0 / 1 / 2 by level, position = words 3 .. 6, background = the last two words (words: split at single
    spaces, so a double space makes an empty word).  A caption too short for the place gives None."""
    words = text.split(" ")
    try:
        if attribute in _WORDS_OF:
            part = " ".join([words[i] for i in _WORDS_OF[attribute]])
        else:
            part = words[_WORD_OF[attribute][level]]
    except IndexError:
        return None
    return _first_contained(SEARCH_ORDER[attribute], part)


def retrieve_attributes(text, level):
    """the attribute values of a decoded caption joined by spaces, UNKNOWN where none is spelled (joint coherence)"""
    vals = [attribute_in_decoded(a, text, level) for a in _level_attributes(level)]
    return " ".join(UNKNOWN if v is None else v for v in vals)


def count_same_letters(a, b):
    """positions at which two strings agree, over the length of the shorter one"""
    return sum(1 for x, y in zip(a, b) if x == y)


def score_decoded_text(level, caption, decoded):
    """Image -> Text: (strict, features, letters) of one decoded caption against its ground truth.
    features: share of the level's attributes whose decoded value occurs in the caption (substring);
    letters: matching positions / len(caption);  strict: 1 iff letters == 1 (NOT "all attributes")."""
    atts = _level_attributes(level)
    ok = 0
    for a in atts:
        v = attribute_in_decoded(a, decoded, level)
        ok += int(v is not None and v in caption)
    letters = count_same_letters(decoded, caption) / len(caption) if len(caption) else 0.0
    return (1 if letters == 1 else 0), ok / len(atts), letters


def caption_labels(level, caption):
    """Text -> Image: the class index per attribute of the level that the caption asks for; -1 where the caption names no
    value, or one no classifier has a class for ("white")"""
    out = []
    for a in _level_attributes(level):
        v = attribute_in_caption(a, caption)
        out.append(CLASS_NAMES[a].index(v) if v in CLASS_NAMES[a] else -1)
    return out


def mean_stats(lists, percentage=True):
    """the means of several per-sample lists, as percentages"""
    return [(100.0 if percentage else 1.0) * sum(l) / len(l) for l in lists]


# ---- image classifiers ----------------------------------------------------------------------------------------------
def _cache_key(params):
    """changes whenever one of `params` was replaced, moved or written in place: what a packed copy of them is kept under"""
    return tuple((p.data_ptr(), p._version, str(p.device)) for p in params)


class _Wrapped(nn.Module):
    """a layer under the key `<name>.module.*` (the reference wraps every layer in DataParallel)"""

    def __init__(self, module):
        super().__init__()
        self.module = module


class AttributeClassifier(nn.Module):
    """eval/train_classifiers.py: CNN -- four Conv2d(k4, s2, p1) 3->32->32->32->32 with ReLU, Linear 512->256 + ReLU,
    Linear 256->n_classes, under the reference's state-dict keys (conv1 / conv2 / conv3 / conv_64 / lin1 / lin2 /
    fc, each `.module.weight|bias`; lin2 is carried and unused, as there), so its shipped classifier files load with
    strict=True.  Inference only: the trunk runs on ops.conv2d (the ReLU of layer l applied by layer l + 1 while it
    stages its input), the head on ops.cls_head."""

    def __init__(self, n_classes):
        super().__init__()
        n_classes = int(n_classes)
        if not 2 <= n_classes <= H.COH_MAX_CLASSES:
            raise ValueError(f"AttributeClassifier: {n_classes} classes (2 .. {H.COH_MAX_CLASSES} are on the MI355X path)")
        self.n_classes = n_classes
        conv = lambda cin: _Wrapped(nn.Conv2d(cin, 32, 4, stride=2, padding=1))
        self.conv1, self.conv2, self.conv3, self.conv_64 = conv(3), conv(32), conv(32), conv(32)
        self.lin1 = _Wrapped(nn.Linear(H.COH_FEATS, H.COH_HIDDEN))
        self.lin2 = _Wrapped(nn.Linear(H.COH_HIDDEN, H.COH_HIDDEN))
        self.fc = _Wrapped(nn.Linear(H.COH_HIDDEN, n_classes))
        self.requires_grad_(False)

    def trunk(self, x):
        """x (N,3,64,64) -> (N,512): the fourth conv's output before its ReLU, flattened (channel, y, x)"""
        with torch.no_grad():
            act = H.ACT_NONE
            for layer in (self.conv1, self.conv2, self.conv3, self.conv_64):
                x = ops.conv2d(x, layer.module.weight, layer.module.bias, 2, 1, act)
                act = H.ACT_RELU
            return x.reshape(x.shape[0], -1)

    def forward(self, x):
        """logits (N, n_classes) of images x (N,3,64,64) in [0, 1]"""
        return AttributeClassifiers({"_": self}).predict(x, quantise=False, want_logits=True)["logits"][0]


def attribute_features(classifier):
    """an AttributeClassifier's 512-d trunk as a feature extractor of TorchMMVAE.frechet_distances: x -> (N, 512).  The
    images are taken as they are -- no 8-bit quantisation, as the reference's FID path takes tensors (and floor(255 x) on
    real data stored as k / 255 can land on k - 1)."""
    if not isinstance(classifier, AttributeClassifier):
        raise TypeError(f"attribute_features: a {type(classifier).__name__}, not an AttributeClassifier")
    return lambda x: classifier.trunk(x.detach().float().reshape(-1, 3, 64, 64).contiguous())


def quantise_images(x_hat):
    """a decoder output in [0, 1] as the reference's pipeline hands it to the classifiers: x 255, cast to uint8
    (truncation), / 255 -- floor(255 x) / 255 in fp32 -- and reinterpreted (not permuted) as (N,3,64,64)"""
    x = torch.floor(x_hat.detach().float() * 255.0).clamp_(0.0, 255.0) / 255.0
    return x.reshape(-1, 3, 64, 64)


class AttributeClassifiers(nn.Module):
    """{attribute: AttributeClassifier}, scored together: A trunks, ONE head launch"""

    def __init__(self, classifiers):
        super().__init__()
        if not classifiers or len(classifiers) > H.COH_MAX_CLASSIFIERS:
            raise ValueError(f"AttributeClassifiers: {len(classifiers)} classifiers (1 .. {H.COH_MAX_CLASSIFIERS} per launch)")
        for k, c in classifiers.items():
            if not isinstance(c, AttributeClassifier):
                raise TypeError(f"AttributeClassifiers: {k!r} is a {type(c).__name__}, not an AttributeClassifier")
        self.nets = nn.ModuleDict(classifiers)
        self._packed = None

    @classmethod
    def for_level(cls, level):
        """untrained classifiers of a level's attributes with the reference's class counts (load their state dicts)"""
        return cls({a: AttributeClassifier(len(CLASS_NAMES[a])) for a in _level_attributes(level)})

    @property
    def attributes(self):
        return list(self.nets.keys())

    @property
    def n_classes(self):
        return [c.n_classes for c in self.nets.values()]

    def packed_head(self):
        """(W1 (A,256,512), b1 (A,256), W2 (A,Cmax,256), b2 (A,Cmax)); packed again whenever a head parameter was
        replaced, moved or written in place"""
        nets = list(self.nets.values())
        src = [p for n in nets for p in (n.lin1.module.weight, n.lin1.module.bias, n.fc.module.weight, n.fc.module.bias)]
        key = _cache_key(src)
        if self._packed is None or self._packed[0] != key:
            Cmax = max(self.n_classes)
            dev = src[0].device
            W2 = torch.zeros(len(nets), Cmax, H.COH_HIDDEN, device=dev)
            b2 = torch.zeros(len(nets), Cmax, device=dev)
            for i, n in enumerate(nets):
                W2[i, :n.n_classes] = n.fc.module.weight.detach().float()
                b2[i, :n.n_classes] = n.fc.module.bias.detach().float()
            self._packed = (key, (torch.stack([n.lin1.module.weight.detach().float() for n in nets]).contiguous(),
                                  torch.stack([n.lin1.module.bias.detach().float() for n in nets]).contiguous(), W2, b2))
        return self._packed[1]

    def predict(self, x_hat, labels=None, quantise=True, want_logits=False):
        """x_hat: decoder output, any shape that reshapes to (N,3,64,64), in [0, 1]; labels (A,N) ints or None (-1: never
        correct).  -> ops.cls_head's dict: pred (A,N), logits (A,N,Cmax) | None, correct (A,N), n_correct (N,)"""
        x = quantise_images(x_hat) if quantise else x_hat.detach().float().reshape(-1, 3, 64, 64)
        x = x.contiguous()
        feats = torch.stack([n.trunk(x) for n in self.nets.values()]).contiguous()
        if labels is not None:
            labels = torch.as_tensor(labels).to(device=x.device, dtype=torch.int32).contiguous()
            if labels.shape != (len(self.nets), x.shape[0]):
                raise ValueError(f"AttributeClassifiers.predict: labels {tuple(labels.shape)} for {len(self.nets)} "
                                 f"classifiers and {x.shape[0]} images")
        return ops.cls_head(feats, *self.packed_head(), self.n_classes, labels=labels, want_logits=want_logits)

    def names(self, pred):
        """pred (A,N) -> per image the list of class names, in attribute order"""
        pred = pred.cpu().tolist()
        atts = self.attributes
        return [[CLASS_NAMES[a][pred[i][n]] for i, a in enumerate(atts)] for n in range(len(pred[0]))]


def check_classifiers(classifiers, level):
    """the level's attributes, each with a classifier of the benchmark's class count -> the classifiers in level order"""
    atts = _level_attributes(level)
    if not isinstance(classifiers, AttributeClassifiers):
        raise TypeError("coherence: `classifiers` must be an AttributeClassifiers")
    missing = [a for a in atts if a not in classifiers.nets]
    if missing:
        raise ValueError(f"coherence: level {level} needs classifiers for {list(atts)}; {missing} are missing")
    for a in atts:
        if classifiers.nets[a].n_classes != len(CLASS_NAMES[a]):
            raise ValueError(f"coherence: the {a} classifier has {classifiers.nets[a].n_classes} classes, the benchmark "
                             f"{len(CLASS_NAMES[a])}")
    if classifiers.attributes == list(atts):
        return classifiers
    return AttributeClassifiers({a: classifiers.nets[a] for a in atts})


def score_images(classifiers, level, x_hat, captions):
    """Text -> Image / joint: classify the decoded images against what the captions name.
    -> (strict (N,) 0/1 list, features (N,) list of fractions, the cls_head dict)"""
    atts = _level_attributes(level)
    labels = torch.tensor([caption_labels(level, c) for c in captions], dtype=torch.int32).t().contiguous()
    out = classifiers.predict(x_hat, labels=labels)
    n_ok = out["n_correct"].cpu().tolist()
    return [int(k == len(atts)) for k in n_ok], [k / len(atts) for k in n_ok], out


# ---- MNIST-SVHN digit classifiers (eval/mnistsvhn_helper.py:191-226, eval/eval_mnistsvhn.py:70-120) ---------------------
class DigitClassifier(nn.Module):
    """eval/mnistsvhn_helper.py: MNIST_Classifier / SVHN_Classifier -- Conv2d(C, 10, 5), max-pool 2, ReLU, Conv2d(10, 20, 5),
    Dropout2d, max-pool 2, ReLU, Linear(320 | 500, 50), ReLU, dropout, Linear(50, 10), log_softmax -- under the
    reference's state-dict keys (conv1 / conv2 / fc1 / fc2, each `.weight|bias`), so a mnist_model.pt / svhn_model.pt it
    wrote loads with strict=True.  The modules only hold the parameters: forward and training run on csrc/digits.hip
    (ops.digit_eval / ops.digit_train through DigitClassifiers)."""

    def __init__(self, kind):
        super().__init__()
        if kind not in ops.DIGIT_KINDS:
            raise ValueError(f"DigitClassifier: kind = {kind!r} ('mnist' or 'svhn')")
        self.kind = kind
        C, flat = ops.DIGIT_INPUT[kind][0], (320 if kind == "mnist" else 500)
        self.conv1 = nn.Conv2d(C, 10, kernel_size=5)
        self.conv2 = nn.Conv2d(10, 20, kernel_size=5)
        self.fc1 = nn.Linear(flat, 50)
        self.fc2 = nn.Linear(50, 10)
        self.requires_grad_(False)
        self._packed = None

    def packed_state(self):
        """(1, 3, n_params) device state whose first row holds the packed parameters; packed again whenever a parameter was
        replaced, moved or written in place"""
        src = [self.get_parameter(k) for k, _ in ops.digit_param_shapes(self.kind)]
        key = _cache_key(src)
        if self._packed is None or self._packed[0] != key:
            st = torch.zeros(1, 3, ops.DIGIT_N_PARAMS[self.kind], device=src[0].device)
            st[0, 0] = torch.cat([p.detach().float().reshape(-1) for p in src])
            self._packed = (key, st)
        return self._packed[1]

    def images(self, x):
        """any tensor that holds (N,C,H,W) images -- or (N,32,32,3), as Dec_SVHN returns them: permuted back -- as the
        contiguous fp32 (N,C,H,W) the kernels read"""
        C, Hh, Ww = ops.DIGIT_INPUT[self.kind]
        x = x.detach().float()
        if C == 3 and tuple(x.shape[-3:]) == (Hh, Ww, C):
            x = x.reshape(-1, Hh, Ww, C).permute(0, 3, 1, 2)
        if x.numel() % (C * Hh * Ww) != 0:
            raise ValueError(f"DigitClassifier({self.kind}): images of shape {tuple(x.shape)}")
        return x.reshape(-1, C, Hh, Ww).contiguous()

    def features(self, x):
        """(N, 50): relu(fc1), the hidden layer, dropout off -- a feature extractor of TorchMMVAE.frechet_distances"""
        return ops.digit_hidden(self.packed_state(), [self.kind], [self.images(x)])[0]

    def forward(self, x):
        """log-probabilities (N, 10) of images x (N,C,H,W); dropout off (the classifiers score in eval mode)"""
        return ops.digit_eval(self.packed_state(), [self.kind], [self.images(x)])[0][0]


class DigitClassifiers(nn.Module):
    """The MNIST and the SVHN digit classifier of the MNIST-SVHN coherence metrics, trained and scored together."""
    KINDS = ("mnist", "svhn")

    def __init__(self, mnist=None, svhn=None):
        super().__init__()
        mnist = DigitClassifier("mnist") if mnist is None else mnist
        svhn = DigitClassifier("svhn") if svhn is None else svhn
        for k, c in (("mnist", mnist), ("svhn", svhn)):
            if not isinstance(c, DigitClassifier) or c.kind != k:
                raise TypeError(f"DigitClassifiers: `{k}` must be a DigitClassifier('{k}')")
        self.mnist, self.svhn = mnist, svhn
        self._stacked = None

    def _split(self, batches, what, mnist=None, svhn=None):
        """an iterable of (batch dict, labels) -> (MNIST images (N,1,28,28), SVHN images (N,3,32,32), labels (N,) int32),
        on the classifiers' device.  The modalities are `mnist` / `svhn`, else the ones whose rows hold 784 / 3072 values."""
        batches = list(batches)
        y = ops.label_matrix(batches, what, "DigitClassifiers")
        if y.shape[0] != 1:
            raise ValueError(f"DigitClassifiers: {y.shape[0]} label columns in the {what} set (one digit label per sample)")
        if int(y.min()) < 0 or int(y.max()) >= 10:
            raise ValueError(f"DigitClassifiers: {what} labels in [{int(y.min())}, {int(y.max())}], outside [0, 10)")
        dev = self.mnist.conv1.weight.device
        xs = {"mnist": [], "svhn": []}
        for batch, _ in batches:
            names = {"mnist": mnist, "svhn": svhn}
            for k, n_el in (("mnist", 784), ("svhn", 3072)):
                if names[k] is None:
                    hit = [m for m, v in batch.items() if v["data"] is not None and v["data"][0].numel() == n_el]
                    if len(hit) != 1:
                        raise ValueError(f"DigitClassifiers: name the `{k}` modality (batch holds {list(batch)})")
                    names[k] = hit[0]
                if names[k] not in batch or batch[names[k]]["data"] is None:
                    raise ValueError(f"DigitClassifiers: a {what} batch has no data for modality {names[k]!r}")
                xs[k].append(getattr(self, k).images(batch[names[k]]["data"]).to(dev))
        xm, xsv = torch.cat(xs["mnist"]).contiguous(), torch.cat(xs["svhn"]).contiguous()
        if xm.shape[0] != y.shape[1] or xsv.shape[0] != y.shape[1]:
            raise ValueError(f"DigitClassifiers: {xm.shape[0]} MNIST / {xsv.shape[0]} SVHN images for {y.shape[1]} labels")
        return xm, xsv, y[0].to(device=dev, dtype=torch.int32).contiguous()

    def _stacked_state(self):
        """(2, 3, n_params_max) state with both networks' packed parameters, built again only when one of them was"""
        packed = [n.packed_state() for n in (self.mnist, self.svhn)]
        key = tuple(id(p) for p in packed)
        if self._stacked is None or self._stacked[0] != key:
            st = torch.zeros(2, 3, ops.DIGIT_N_PARAMS["svhn"], device=packed[0].device)
            for i, p in enumerate(packed):
                st[i, 0, :p.shape[-1]] = p[0, 0]
            self._stacked = (key, st, packed)
        return self._stacked[1]

    def fit(self, train, epochs, batch_size=128, lr=1e-3, seed=0, p=0.5, shuffle=False, mnist=None, svhn=None):
        """The reference's training loop (eval/eval_mnistsvhn.py:76-97: CrossEntropyLoss + optim.Adam(lr), minibatches in
        the loader's order) for both classifiers side by side, from the parameters the modules hold.  `train`: an iterable
        of (batch dict, labels (B,) ints) as TorchMMVAE.classify_latents takes it.  The images are copied to the device
        once; every epoch is one ops.digit_train call (`shuffle`: per-epoch permutations from torch.Generator(seed));
        `seed` also keys the dropout masks, `p` is their rate (the reference's 0.5).
        -> loss (2, steps): the mean loss of every step, rows mnist / svhn; the trained parameters are written back."""
        epochs, batch_size = int(epochs), int(batch_size)
        if epochs < 1 or batch_size < 1:
            raise ValueError(f"DigitClassifiers.fit: epochs = {epochs}, batch_size = {batch_size}")
        xm, xs, y = self._split(train, "train", mnist, svhn)
        dev, N = xm.device, xm.shape[0]
        nets = [self.mnist, self.svhn]
        state = ops.digit_state(self.KINDS, dev, init=[{k: v for k, v in n.state_dict().items()} for n in nets])
        order = ops.epoch_orders(N, epochs, seed, dev, shuffle)
        spe = (N + batch_size - 1) // batch_size
        curve = torch.cat([ops.digit_train(state, self.KINDS, [xm, xs], [y, y], batch_size, e * spe, spe, lr=lr, seed=seed,
                                           p=p, order=order, validate=False) for e in range(epochs)], 1)
        with torch.no_grad():
            for i, n in enumerate(nets):
                for k, v in ops.digit_unpack(n.kind, state[i, 0]).items():
                    n.get_parameter(k).copy_(v)
        return curve

    def predict(self, x_mnist=None, x_svhn=None):
        """the digits the classifiers see: -> {"mnist": (N,) int32 | absent, "svhn": ...} (first maximum of the
        log-probabilities); both networks in one launch when both image sets have the same length"""
        if x_mnist is None and x_svhn is None:
            raise ValueError("DigitClassifiers.predict: no images")
        given = [(k, getattr(self, k), x) for k, x in (("mnist", x_mnist), ("svhn", x_svhn)) if x is not None]
        imgs = [n.images(x) for _, n, x in given]
        if len(given) == 2 and imgs[0].shape[0] == imgs[1].shape[0]:
            pred = ops.digit_eval(self._stacked_state(), list(self.KINDS), imgs)[1]
            return {k: pred[i] for i, k in enumerate(self.KINDS)}
        return {k: ops.digit_eval(n.packed_state(), [k], [x])[1][0] for (k, n, _), x in zip(given, imgs)}

    def accuracy(self, test, mnist=None, svhn=None):
        """-> {"mnist": share of the test images classified as their label, "svhn": ...} (fractions in [0, 1])"""
        xm, xs, y = self._split(test, "test", mnist, svhn)
        pred = self.predict(xm, xs)
        return {k: float((pred[k] == y).sum()) / y.shape[0] for k in self.KINDS}


# ---- sentence features for the cross-modal correlation (reference: eval/mnistsvhn_helper.py:116-177) ------------------------
def sif_weights(counts, a=1e-3):
    """the tokens' smooth-inverse-frequency weights a / (a + count / total) from their occurrence counts (V,), float32"""
    counts = torch.as_tensor(counts, dtype=torch.float64)
    if counts.dim() != 1 or counts.numel() < 1 or bool((counts < 0).any()) or float(counts.sum()) <= 0 or not a > 0:
        raise ValueError("sif_weights: counts are non-negative occurrence counts (V,) with a positive total; a > 0")
    return (a / (a + counts / counts.sum())).float()


class SentenceFeatures:
    """The caption feature of the cross-modal correlation: the frequency-weighted mean of a caption's word embeddings up to
    its first `eos` token, with the captions' common component removed once `fit_pc` has found it (ops.sentence_features).
    `emb` (V, E) is the caller's embedding table (the reference trains FastText on the captions; it cannot be shipped),
    `weights` (V,) the tokens' weights (sif_weights).  Callable on (B, T, V) one-hot rows or probabilities (the argmax over V
    is the token) or on (B, T) integer ids -> (B, E) fp32 features on the table's device."""

    def __init__(self, emb, weights, eos=2):
        if not torch.is_tensor(emb) or emb.dim() != 2 or not torch.is_tensor(weights) or tuple(weights.shape) != emb.shape[:1]:
            raise ValueError("SentenceFeatures: emb is the (V, E) embedding table, weights (V,) one weight per token")
        self.emb, self.weights, self.eos, self.pc = emb, weights, int(eos), None

    def ids(self, text):
        if not torch.is_tensor(text) or text.dim() not in (2, 3):
            raise ValueError("SentenceFeatures: captions are (B, T, V) one-hot rows or probabilities, or (B, T) ids")
        if text.dim() == 3:
            if text.shape[2] != self.emb.shape[0]:
                raise ValueError(f"SentenceFeatures: captions over {text.shape[2]} tokens, the table holds {self.emb.shape[0]}")
            text = text.argmax(dim=2)
        return text

    def __call__(self, text):
        return ops.sentence_features(self.ids(text), self.emb, self.weights, self.eos, self.pc)

    def unprojected(self, text):
        """the features with the common component left in (what fit_pc works on)"""
        return ops.sentence_features(self.ids(text), self.emb, self.weights, self.eos, None)

    def fit_pc(self, texts):
        """`texts`: an iterable of caption batches.  Sets and returns `pc` (E,) float64: the top eigenvector of the
        covariance of their features without the projection (streamed moments, ops.sym_eig) -- the reference's top right
        singular vector of the centred feature matrix up to sign, which the projection f - pc (pc . f) does not see."""
        state = None
        for text in texts:
            f = self.unprojected(text)
            state = ops.frechet_state(f.shape[1], f.device) if state is None else state
            ops.frechet_update(state, f)
        if state is None:
            raise ValueError("SentenceFeatures.fit_pc: `texts` is empty")
        _, _, sigma = ops.frechet_moments(state)
        e = ops.sym_eig(sigma)
        v = e["vectors"][:, int(e["values"].argmax())]
        self.pc = (v / torch.linalg.vector_norm(v)).contiguous()
        return self.pc
