"""Plain Python / numpy restatement of the text generation quality, written from the definitions: the
cut by length, end marker and trailing filler, the two alignments as row-by-row dynamic programmes over the whole table, the
clipped n-gram matches from collections.Counter, words as tuples of tokens, the negative log-likelihood in float64 -- and the
summary figures in plain Python.  Nothing is shared with csrc/text_quality.hip or ops.text_quality_summary.

Every count is an integer and is held exactly.  The one float, nll = sum_{t < S} (m_t + log s_t - x_t[ref_t]) with
s_t = sum_v exp(x_v - m_t), carries a bar derived from the arithmetic, not measured: with u = 2^-53, correctly rounded sums and
exp / log within 2 ulp, s_t (V terms in (0, 1], each exp off by <= 4 u, V - 1 additions) is off by <= (V + 3) u s_t relatively
in any order, so log s_t by <= (V + 3) u + 4 u |log s_t|; the step's two additions add 2 u (|m_t| + |log s_t| + |x_t|) and the
S - 1 additions of the steps, in any order, (S - 1) u sum_t (|m_t| + |log s_t| + |x_t|).  Two evaluations each inside that differ
by at most twice it, which bar[n] = 2^-52 [(V + 8) S + (S + 8) sum_{t < S} (|m_t| + |log s_t| + |x_t|)] covers; S = 0 gives 0."""
import collections
import functools
import math

import numpy as np

TOKEN_KEYS = ("hyp_len", "ref_len", "same", "edit", "lcs", "match", "total")
WORD_KEYS = ("hyp_len", "ref_len", "edit", "lcs", "match", "total")
MAX_ORDER = 4


# ---- stages 2 - 4 for one pair -------------------------------------------------------------------------------------------------------
def cut(seq, length, eos=None, trim=None):
    """seq[: clamp(length, 0, len(seq))], ended before its first eos, then without its trailing trims -> list of ints"""
    s = [int(v) for v in seq[:min(max(int(length), 0), len(seq))]]
    if eos is not None and eos in s:
        s = s[:s.index(eos)]
    if trim is not None:
        while s and s[-1] == trim:
            s.pop()
    return s


def levenshtein(a, b):
    """unit-cost edit distance, row by row over the whole (len(a) + 1) x (len(b) + 1) table"""
    j = np.arange(len(b) + 1)
    row = j.copy()
    for i, tok in enumerate(a, 1):
        differ = np.array([x != tok for x in b], dtype=np.int64)      # (tokens are ints, words tuples of ints)
        new = np.empty_like(row)
        new[0] = i
        new[1:] = np.minimum(row[1:] + 1, row[:-1] + differ)          # from above, from the diagonal
        row = np.minimum.accumulate(new - j) + j                      # from the left: new[j] = min_k<=j new[k] + (j - k)
    return int(row[-1])


def lcs(a, b):
    """length of the longest common subsequence, row by row"""
    row = np.zeros(len(b) + 1, dtype=np.int64)
    for tok in a:
        equal = np.array([x == tok for x in b], dtype=np.int64)
        new = row.copy()                                              # from above
        new[1:] = np.maximum(new[1:], (row[:-1] + 1) * equal)         # a match extends the diagonal
        row = np.maximum.accumulate(new)                              # from the left
    return int(row[-1])


def ngrams(s, n):
    return collections.Counter(tuple(s[i:i + n]) for i in range(len(s) - n + 1))


def clipped(h, r, K):
    """(match, total) of orders 1 .. 4, zero beyond K: Papineni's clipped counts"""
    match, total = [0] * MAX_ORDER, [0] * MAX_ORDER
    for n in range(1, K + 1):
        ch, cr = ngrams(h, n), ngrams(r, n)
        match[n - 1] = sum(min(c, cr[g]) for g, c in ch.items())
        total[n - 1] = max(len(h) - n + 1, 0)
    return match, total


def words(s, sep):
    """the maximal runs of tokens != sep, as tuples"""
    out, run = [], []
    for tok in s:
        if tok == sep:
            if run:
                out.append(tuple(run))
            run = []
        else:
            run.append(tok)
    if run:
        out.append(tuple(run))
    return out


def level(h, r, K, same):
    m, t = clipped(h, r, K)
    out = {"hyp_len": len(h), "ref_len": len(r), "edit": levenshtein(h, r), "lcs": lcs(h, r), "match": m, "total": t}
    if same:
        out["same"] = sum(int(x == y) for x, y in zip(h, r))
    return out


# ---- stage 1 and the whole call ------------------------------------------------------------------------------------------------------
def decode(logits, ref_ids, ref_lengths):
    """logits (N, Th, V) fp32 -> pred (N, Th) (the first maximum), nll (N,) float64, nll_steps (N,), bar (N,)"""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    N, Th, V = x.shape
    Tr = ref_ids.shape[1]
    pred = np.argmax(x, axis=-1).astype(np.int32)      # (numpy returns the first of equal maxima)
    m = x.max(-1)
    s = np.zeros((N, Th))
    for v in range(V):
        s += np.exp(x[:, :, v] - m)
    nll, steps, bar = np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros(N)
    for n in range(N):
        S = min(min(max(int(ref_lengths[n]), 0), Tr), Th)
        mag = 0.0
        for t in range(S):
            xt = x[n, t, int(ref_ids[n, t])]
            nll[n] += (m[n, t] + math.log(s[n, t])) - xt
            mag += abs(m[n, t]) + abs(math.log(s[n, t])) + abs(xt)
        steps[n] = S
        bar[n] = 2.0 ** -52 * ((V + 8) * S + (S + 8) * mag)
    return pred, nll, steps, bar


def text_quality(hyp, ref_ids, ref_lengths, hyp_lengths=None, eos=None, trim=None, sep=None, max_order=4):
    """the outputs of ops.text_quality as numpy arrays, and "bar" (N,) for nll"""
    hyp, ref_ids = np.asarray(hyp), np.asarray(ref_ids)
    N, Th = hyp.shape[:2]
    pred = nll = steps = bar = None
    ids = hyp
    if hyp.ndim == 3:
        pred, nll, steps, bar = decode(hyp, ref_ids, ref_lengths)
        ids = pred
    tok = {k: [] for k in TOKEN_KEYS}
    wrd = {k: [] for k in WORD_KEYS} if sep is not None else None
    for n in range(N):
        h = cut(ids[n], Th if hyp_lengths is None else hyp_lengths[n], eos, trim)
        r = cut(ref_ids[n], ref_lengths[n], eos, trim)
        for k, v in level(h, r, max_order, True).items():
            tok[k].append(v)
        if wrd is not None:
            for k, v in level(words(h, sep), words(r, sep), max_order, False).items():
                wrd[k].append(v)
    arr = lambda d: None if d is None else {k: np.asarray(v, dtype=np.int32) for k, v in d.items()}
    return {"token": arr(tok), "word": arr(wrd), "pred": pred, "nll": nll, "nll_steps": steps, "bar": bar,
            "max_order": max_order}


# ---- the summary, in plain Python ----------------------------------------------------------------------------------------------------
def level_summary(c, K, token):
    """c: {name: per-pair lists / arrays}"""
    n = len(c["edit"])
    H, R = sum(int(v) for v in c["hyp_len"]), sum(int(v) for v in c["ref_len"])
    M = [sum(int(row[k]) for row in c["match"]) for k in range(K)]
    T = [sum(int(row[k]) for row in c["total"]) for k in range(K)]
    bp = lambda h, r: math.exp(1.0 - r / h) if h < r else 1.0
    bleu = 0.0
    if H > 0 and all(m > 0 for m in M):
        bleu = bp(H, R) * math.exp(sum(math.log(m / t) for m, t in zip(M, T)) / K)
    sent, rouge = 0.0, 0.0
    for i in range(n):
        h, r, l = int(c["hyp_len"][i]), int(c["ref_len"][i]), int(c["lcs"][i])
        m, t = [int(v) for v in c["match"][i]], [int(v) for v in c["total"][i]]
        if h > 0 and m[0] > 0:
            p = [m[0] / t[0]] + [(m[k] + 1) / (t[k] + 1) for k in range(1, K)]
            sent += bp(h, r) * math.exp(sum(math.log(v) for v in p) / K)
        P, Rc = (l / h if h else 0.0), (l / r if r else 0.0)
        rouge += 2.0 * P * Rc / (P + Rc) if P + Rc > 0.0 else 0.0
    E = sum(int(v) for v in c["edit"])
    out = {"n": n, "error_rate": E / R if R else (0.0 if E == 0 else math.inf),
           "exact": sum(int(v) == 0 for v in c["edit"]) / n, "bleu": bleu,
           "precisions": [m / t if t else 0.0 for m, t in zip(M, T)], "sentence_bleu": sent / n, "rouge_l": rouge / n}
    if token:
        out["accuracy"] = sum(int(v) for v in c["same"]) / R if R else 0.0
    return out


def summary(parts):
    """text_quality_summary of a list of text_quality results (numpy or lists)"""
    K = parts[0]["max_order"]
    join = lambda name: None if parts[0][name] is None else {k: [v for p in parts for v in np.asarray(p[name][k]).tolist()]
                                                             for k in parts[0][name]}
    token = level_summary(join("token"), K, True)
    word = None if parts[0]["word"] is None else level_summary(join("word"), K, False)
    if parts[0]["nll"] is None:
        token.update(nll=None, perplexity=None, bits_per_token=None)
    else:
        steps = sum(int(v) for p in parts for v in np.asarray(p["nll_steps"]).tolist())
        total = math.fsum(float(v) for p in parts for v in np.asarray(p["nll"]).tolist())
        mean = total / steps if steps else math.nan
        token.update(nll=mean, perplexity=math.exp(mean), bits_per_token=mean / math.log(2.0))
    return {"token": token, "word": word}


def assert_same_summary(got, want):
    """the figures are short float64 expressions of the same integers: they agree to a few roundings of their logarithms and
    means (16 u relative), and exactly where they are single quotients"""
    assert set(got) == set(want) == {"token", "word"}
    for lvl in ("token", "word"):
        g, w = got[lvl], want[lvl]
        if w is None:
            assert g is None
            continue
        assert set(g) == set(w), (lvl, set(g) ^ set(w))
        for k in w:
            if k in ("n", "error_rate", "exact", "accuracy", "precisions") or w[k] is None:
                assert g[k] == w[k], (lvl, k, g[k], w[k])
            else:
                assert (math.isnan(g[k]) and math.isnan(w[k])) or abs(g[k] - w[k]) <= 16 * 2.0 ** -53 * max(abs(w[k]), 1.0), \
                    (lvl, k, g[k], w[k])


# ---- the shared cases ----------------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 255, 256)


def noisy(r, rng, V, p=0.12):
    """a copy of r with substitutions, insertions and deletions"""
    out = []
    for tok in r:
        u = rng.random()
        if u < p:
            out.append(int(rng.integers(V)))
        elif u < 2 * p:
            out += [int(tok), int(rng.integers(V))]
        elif u < 3 * p:
            continue
        else:
            out.append(int(tok))
    return out


def fit(seq, T, fill=0):
    return (list(seq) + [fill] * T)[:T]


def as_logits(ids, V, rng, margin=3.0):
    """fp32 logits (N, T, V) whose argmax is `ids`: unit normal noise, the chosen id lifted 0.5 .. 0.5 + margin above the
    row's maximum"""
    ids = np.asarray(ids)
    x = rng.standard_normal(ids.shape + (V,)).astype(np.float32)
    top = x.max(-1)
    np.put_along_axis(x, ids[..., None], (top + np.float32(margin) * rng.random(ids.shape).astype(np.float32)
                                          + np.float32(0.5))[..., None], axis=-1)
    assert np.array_equal(np.argmax(x, -1), ids)
    return x


def _pairs(N, Th, Tr, V, rng, alphabet=None):
    """N references of random lengths over `alphabet` symbols (plenty of separators 0) and noisy copies as hypotheses"""
    A = alphabet or min(V, 6)
    ref, hyp, rl, hl = [], [], [], []
    for _ in range(N):
        L = int(rng.integers(0, Tr + 1))
        r = [int(v) for v in rng.integers(0, A, L)]
        h = noisy(r, rng, A)[:Th]
        ref.append(fit(r, Tr))
        hyp.append(fit(h, Th))
        rl.append(L)
        hl.append(len(h))
    return (np.array(hyp, dtype=np.int64), np.array(ref, dtype=np.int64), np.array(rl, dtype=np.int64),
            np.array(hl, dtype=np.int64))


def _edge_lengths():
    """every pair of the edge lengths on either side, T = 256, ids form, words on"""
    rng = np.random.default_rng(1)
    hyp, ref, rl, hl = [], [], [], []
    for a in EDGE_LENGTHS:
        for b in EDGE_LENGTHS:
            r = [int(v) for v in rng.integers(0, 5, 256)]
            h = fit(noisy(r, rng, 5), 256, fill=1)
            hyp.append(h)
            ref.append(r)
            hl.append(a)
            rl.append(b)
    return dict(hyp=np.array(hyp), ref=np.array(ref), ref_len=np.array(rl), hyp_len=np.array(hl), kw=dict(sep=0))


def _logits_case(N, Th, Tr, V, seed, lengths=False, **kw):
    rng = np.random.default_rng(seed)
    hyp, ref, rl, hl = _pairs(N, Th, Tr, V, rng)
    return dict(hyp=as_logits(hyp, V, rng), ref=ref, ref_len=rl, hyp_len=hl if lengths else None, kw=kw)


def _shapes_of_text():
    """identical sequences, sequences that share no token, one repeated token (Papineni's clipping example), in one call"""
    T = 37
    the, cat, is_, on, mat = 1, 2, 3, 4, 5
    rng = np.random.default_rng(3)
    a = [int(v) for v in rng.integers(0, 7, T)]
    rows = [(a, T, a, T),                                                              # identical
            ([1, 2, 3] * 12, 36, [4, 5, 6, 7] * 9, 36),                                # nothing in common
            ([the] * 7, 7, [the, cat, is_, on, the, mat], 6),                          # the the the the the the the
            ([2] * T, T, [2, 0, 2, 2, 0, 2], 6),                                       # one repeated token, longer than the reference
            ([5, 0, 5, 0, 5, 0, 5], 7, [5] * T, T)]
    return dict(hyp=np.array([fit(h, T) for h, _, _, _ in rows]), ref=np.array([fit(r, T) for _, _, r, _ in rows]),
                ref_len=np.array([rl for _, _, _, rl in rows]), hyp_len=np.array([hl for _, hl, _, _ in rows]), kw=dict(sep=0))


def _ties():
    """logits on a grid of four values, so that most rows hold equal maxima (the first index wins), and all-zero rows"""
    rng = np.random.default_rng(5)
    N, T, V = 6, 70, 27
    x = rng.integers(0, 4, (N, T, V)).astype(np.float32)
    x[:, ::5] = 0.0
    x[2] = 0.0
    assert (np.sum(x == x.max(-1, keepdims=True), -1) > 1).mean() > 0.5
    ref = rng.integers(0, V, (N, T))
    return dict(hyp=x, ref=ref, ref_len=rng.integers(0, T + 1, N), hyp_len=None, kw=dict(trim=0, sep=0))


def _eos_trim():
    """eos at position 0, in the middle and absent; a trim that empties a sequence; trailing filler after the cut"""
    T, eos = 20, 3
    rows = [([3, 1, 2, 1], 4, [1, 2, 1, 3], 4),                    # eos first: an empty hypothesis
            ([1, 2, 4, 1, 2], 5, [1, 2, 4, 1, 2], 5),              # no eos
            ([1, 2, 0, 0, 3, 5, 5], 7, [1, 2, 3, 5], 4),           # filler before the eos is trimmed after the cut
            ([0] * T, T, [1, 0, 2], 3),                            # a hypothesis of filler only
            ([1, 0, 2], 3, [0] * T, T),                            # a reference of filler only
            ([0, 0, 3, 1], 4, [3], 1),                             # both empty
            ([1, 4, 0, 2, 0, 0], 6, [1, 4, 0, 2, 3, 1], T)]        # a reference length beyond the eos
    return dict(hyp=np.array([fit(h, T) for h, _, _, _ in rows]), ref=np.array([fit(r, T) for _, _, r, _ in rows]),
                ref_len=np.array([rl for _, _, _, rl in rows]), hyp_len=np.array([hl for _, hl, _, _ in rows]),
                kw=dict(eos=eos, trim=0, sep=0))


def _words():
    """separators leading, trailing and doubled; one 256-token word; 128 one-token words; separators only; repeated words"""
    T = 256
    rng = np.random.default_rng(7)
    one = [int(v) for v in rng.integers(1, 9, T)]
    other = list(one)
    other[100] = other[100] % 8 + 1
    singles = [v for i in range(128) for v in (1 + i % 3, 0)]            # 128 one-token words
    singles2 = [v for i in range(128) for v in (1 + (i * i) % 3, 0)]
    rows = [([0, 0, 1, 2, 0, 0, 3, 0, 4, 4, 0], [1, 2, 0, 3, 0, 0, 4, 4, 0, 0]),
            (one, one), (one, other), (singles, singles2), (singles, one),
            ([0] * T, [1, 2, 0, 3]), ([1, 2, 0, 3], [0] * T), ([0] * 5, [0] * 9),
            ([1, 2, 0] * 85, [1, 2, 0, 2, 1, 0] * 42), ([7, 0, 7, 0, 7, 0, 7], [7, 0, 7])]
    return dict(hyp=np.array([fit(h, T) for h, _ in rows]), ref=np.array([fit(r, T) for _, r in rows]),
                ref_len=np.array([len(r) for _, r in rows]), hyp_len=np.array([len(h) for h, _ in rows]), kw=dict(sep=0))


CASES = [
    ("edge_lengths", _edge_lengths),
    ("logits_45_vs_32", lambda: _logits_case(9, 45, 32, 27, 11, trim=0, sep=0)),
    ("logits_256_vs_7", lambda: _logits_case(5, 256, 7, 27, 12, sep=0)),
    ("logits_7_vs_256", lambda: _logits_case(5, 7, 256, 27, 13, sep=0)),
    ("text_shapes", _shapes_of_text),
    ("vocab_2", lambda: _logits_case(7, 33, 33, 2, 14, sep=0)),
    ("vocab_256", lambda: _logits_case(5, 70, 65, 256, 15, trim=0)),
    ("ties", _ties),
    ("eos_trim", _eos_trim),
    ("hyp_lengths", lambda: _logits_case(9, 129, 129, 27, 16, lengths=True, sep=0)),
    ("words", _words),
    ("order_1", lambda: _logits_case(6, 45, 45, 27, 17, sep=0, max_order=1)),
    ("order_2_ids", lambda: dict(_edge_lengths(), kw=dict(sep=0, max_order=2))),
]
IDS = [name for name, _ in CASES]


@functools.lru_cache(maxsize=None)
def case(i):
    """-> (inputs dict: hyp, ref, ref_len, hyp_len, kw; the restatement's result).  Shared and read-only."""
    c = CASES[i][1]()
    for k in ("hyp", "ref", "ref_len", "hyp_len"):
        if c[k] is not None:
            c[k].setflags(write=False)
    return c, text_quality(c["hyp"], c["ref"], c["ref_len"], c["hyp_len"], **c["kw"])
