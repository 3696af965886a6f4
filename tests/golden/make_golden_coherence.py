"""Generate the generation-coherence fixtures by running the REFERENCE itself (build container only).

    python tests/golden/make_golden_coherence.py

Imports the reference's eval/eval_cdsprites.py and eval/train_classifiers.py under tests/golden/ref_harness.py (which
stubs cv2 / imageio / ...: none of the functions used calls them) and writes, as data only:

  coherence/text_cases.json    (level, caption, decoded caption) tuples with the reference's
                               check_cross_sample_correct(recontext=...) triple, its try_retrieve_atts string and its
                               get_attribute value per attribute of the level;
  coherence/classifier_<k>.npz the parameters of one reference CNN (seeded init, rounded to fp16 and stored as fp16, so
                               that both sides compute with identical fp32 values; lin2, unused in its forward, is left
                               out and zero-filled at load);
  coherence/classifier_cases.npz  12 uint8 images, the reference's logits for both classifiers computed with the module
                               in .double(), and its eval_with_classifier names.
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import numpy as np
import torch

import ref_harness

ref_harness.install()
from eval import eval_cdsprites as ev  # noqa: E402  (the reference module)
from eval.train_classifiers import CNN  # noqa: E402

OUT = os.path.join(HERE, "coherence")

# (level, caption, decoded caption, what the case is about)
TEXT_CASES = [
    # level 1: the label is a bare string
    (1, "heart", "heart", "exact"),
    (1, "square", "squarr", "wrong letter inside the attribute word"),
    (1, "ellipse", "ellipse      ", "trailing spaces from padding"),
    (1, "heart", "hear", "decoded shorter than the caption"),
    (1, "square", "heart", "another value"),
    (1, "ellipse", "xqzv", "unknown word"),
    (1, "heart", " heart", "leading space moves the word"),
    (1, "square", "", "empty decoded caption"),
    # level 2
    (2, "big heart", "big heart", "exact"),
    (2, "small square", "small square   ", "trailing spaces"),
    (2, "big ellipse", "big ellipsa", "wrong letter inside an attribute word"),
    (2, "small heart", "heart small", "swapped word order"),
    (2, "big square", "big", "decoded shorter: no second word"),
    (2, "small ellipse", "small ellipse heart", "decoded longer than the caption"),
    (2, "big heart", "bigg heart", "attribute word as a substring of a longer word"),
    (2, "small heart", "smal heart", "wrong size word"),
    (2, "big square", "big  square", "double space makes an empty word"),
    (2, "small square", "tiny square", "unknown word"),
    (2, "big heart", "small heart", "size differs"),
    # level 3
    (3, "big red heart", "big red heart", "exact"),
    (3, "small blue square", "small blue square     ", "trailing spaces"),
    (3, "big yellow ellipse", "big yellow ellipsf", "wrong letter inside the shape"),
    (3, "small green heart", "small greeb heart", "wrong letter inside the color"),
    (3, "big pink square", "big pink squ", "decoded shorter"),
    (3, "small red ellipse", "small red ellipse at top", "decoded longer"),
    (3, "big blue heart", "blue big heart", "swapped word order"),
    (3, "small yellow square", "small square yellow", "swapped color and shape"),
    (3, "big red heart", "big redd heart", "color as a substring of a longer word"),
    (3, "small white ellipse", "small white ellipse", "a color without a classifier class"),
    (3, "big green square", "big grey square", "unknown color"),
    (3, "small pink heart", "smallpink heart", "missing space"),
    (3, "big red square", "bigredsquare", "no spaces at all"),
    (3, "small blue heart", "small blue hear", "last letter missing"),
    (3, "big blue ellipse", "big blu ellipse", "letter dropped: everything behind it shifts"),
    # level 4
    (4, "big red heart at top left", "big red heart at top left", "exact"),
    (4, "small blue square at bottom right", "small blue square at bottom right   ", "trailing spaces"),
    (4, "big yellow ellipse at top right", "big yellow ellipse at top righ", "wrong letter outside... last letter missing"),
    (4, "small green heart at bottom left", "small green heart at bottom lefx", "wrong letter inside the position"),
    (4, "big pink square at top left", "big pink square at top", "decoded shorter: position words missing"),
    (4, "small red ellipse at top right", "small red ellipse at top right on dark", "decoded longer"),
    (4, "big blue heart at bottom right", "big blue heart bt bottom right", "wrong letter outside an attribute word"),
    (4, "small yellow square at top left", "small yellow square at left top", "swapped position words"),
    (4, "big green ellipse at bottom left", "big green at bottom left ellipse", "shape moved behind the position"),
    (4, "small pink heart at top right", "small pink heart at top rightt", "position as a substring of a longer word"),
    (4, "big red square at bottom right", "big red square at bottom  right", "double space inside the position"),
    (4, "small blue ellipse at top left", "small blue ellipse", "no position at all"),
    (4, "big white heart at top right", "big white heart at top right", "white"),
    (4, "small red square at bottom left", "small red squarf at bottom left", "wrong letter inside the shape"),
    # level 5
    (5, "big red heart at top left on dark", "big red heart at top left on dark", "exact"),
    (5, "small blue square at bottom right on light", "small blue square at bottom right on light   ", "trailing spaces: the last two words are empty"),
    (5, "big yellow ellipse at top right on dark", "big yellow ellipse at top right on darj", "wrong letter inside the background"),
    (5, "small green heart at bottom left on light", "small green heart at bottom left on ligh", "last letter missing"),
    (5, "big pink square at top left on dark", "big pink square at top left on", "decoded shorter: background incomplete"),
    (5, "small red ellipse at top right on light", "small red ellipse at top right on light dark", "decoded longer"),
    (5, "big blue heart at bottom right on dark", "big blue heart at bottom right dark on", "swapped background words"),
    (5, "small yellow square at top left on light", "small yellow square on light at top left", "background before the position"),
    (5, "big green ellipse at bottom left on dark", "big green ellipse at bottom left on darkk", "background as a substring of a longer word"),
    (5, "small pink heart at top right on light", "small pink heart at top right in light", "wrong letter outside an attribute word"),
    (5, "big red square at bottom right on dark", "big red square at bottom right on light", "background differs"),
    (5, "small blue ellipse at top left on light", "small blue ellipse at top left on light", "exact, another sample"),
    (5, "big white heart at top right on dark", "big white heart at top right on dark", "white"),
    (5, "small red square at bottom left on light", "xxxxx xxx xxxxxx xx xxxxxx xxxx xx xxxxx", "nothing recognisable"),
    (5, "big blue heart at top left on dark", "big blue heart", "three words only"),
    (5, "small green square at bottom right on dark", "small green square at bottom right on dar ", "letter lost to a space"),
    (5, "big yellow heart at top left on light", "big yellow hearth at top left on light", "shape as a substring of a longer word"),
    (5, "small pink ellipse at bottom left on dark", "smallpink ellipse at bottom left on dark", "missing space shifts every word"),
    # captions whose own words contain another attribute's value as a substring
    (3, "big red square", "big redsquare", "two attribute words run together"),
    (2, "small square", "smallsquare square", "size word inside the first word with the shape"),
]


GAIN = 2.0      # applied to every weight matrix of the seeded default init


class Exp:
    def __init__(self, level):
        self.level = level


def text_fixture():
    cases = []
    for level, caption, decoded, what in TEXT_CASES:
        exp = Exp(level)
        strict, feats, letters = ev.check_cross_sample_correct(testtext=caption, m_exp=exp, recontext=decoded)
        cases.append({"level": level, "caption": caption, "decoded": decoded, "what": what,
                      "strict": int(strict), "features": float(feats), "letters": float(letters),
                      "retrieved": ev.try_retrieve_atts(decoded, exp),
                      "caption_attributes": {a: ev.get_attribute(a, caption) for a in ev.level_attributes[level]},
                      "retrieved_attributes": {a: ev.get_attribute(a, ev.try_retrieve_atts(decoded, exp))
                                               for a in ev.level_attributes[level]}})
    tables = {"level_attributes": {str(k): v for k, v in ev.level_attributes.items()},
              "class_mappings": ev.class_mappings}
    with open(os.path.join(OUT, "text_cases.json"), "w") as f:
        json.dump({"cases": cases, "tables": tables}, f, indent=1)
    print(f"text_cases.json: {len(cases)} cases")


def classifier_fixture():
    torch.manual_seed(1234)
    g = np.random.default_rng(99)
    images = g.integers(0, 256, size=(12, 3, 64, 64), dtype=np.uint8)
    # smooth half of them a little: a classifier sees blobs, not only noise
    for i in range(0, 12, 2):
        images[i] = g.integers(0, 256, size=(3, 1, 1), dtype=np.uint8)      # a flat background ...
        y, x = g.integers(0, 40, size=2)
        images[i, :, y:y + 24, x:x + 24] = g.integers(0, 256, size=(3, 1, 1), dtype=np.uint8)      # ... with a square on it
    out = {"images": images}
    for att in ("shape", "color"):
        net = CNN(att)
        with torch.no_grad():
            # the default init gives logits that hardly move with the image (the output bias decides every argmax):
            # a gain on the weights makes the 12 images fall into several classes, with margins far above fp32 rounding
            for name, p in net.named_parameters():
                if name.endswith("weight"):
                    p.mul_(GAIN)
            for p in net.parameters():
                p.copy_(p.half().float())
        sd = {k: v.detach().half().numpy() for k, v in net.state_dict().items() if not k.startswith("lin2.")}
        np.savez(os.path.join(OUT, f"classifier_{att}.npz"), **sd)
        names = [ev.eval_with_classifier(net, images[i], att) for i in range(12)]
        # the module in .double(): its forward() casts the input with .float(); keep that cast at double for this call
        net.double()
        orig = torch.Tensor.float
        torch.Tensor.float = lambda self, *a, **k: self.double()
        try:
            with torch.no_grad():
                x = (torch.tensor(images).to(torch.float32) / 255).double()
                logits = net.forward(x)
        finally:
            torch.Tensor.float = orig
        assert logits.dtype == torch.float64
        assert [ev.class_mappings[att][int(i)] for i in logits.argmax(-1)] == names
        out[f"logits_{att}"] = logits.numpy()
        out[f"names_{att}"] = np.array(names)
        print(att, "classes", net.output_dim, "names", names)
    np.savez(os.path.join(OUT, "classifier_cases.npz"), **out)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    text_fixture()
    classifier_fixture()
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))
