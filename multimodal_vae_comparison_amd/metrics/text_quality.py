"""Text generation quality (csrc/text_quality.hip): edit distance, BLEU and ROUGE-L counts, NLL; forward only."""
import math

import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["text_quality_plan", "text_quality", "text_quality_summary"]


def text_quality_plan(Th, Tr, V, eos=None, trim=None, sep=None, max_order=4):
    """text_quality's checks of its arguments against the sequences' steps Th (hypothesis), Tr (reference) and the
    vocabulary V, before any device call: ValueError, or -> {"eos", "trim", "sep": ids, -1 for None; "max_order"}"""
    who = "text_quality"
    Th, Tr, V, K = int(Th), int(Tr), int(V), int(max_order)
    if not (1 <= Th <= H.TQ_MAX_STEPS and 1 <= Tr <= H.TQ_MAX_STEPS):
        raise ValueError(f"{who}: hypotheses of {Th} steps, references of {Tr} (1 .. {H.TQ_MAX_STEPS} steps are on the MI355X "
                         f"path)")
    if not 2 <= V <= H.TQ_MAX_VOCAB:
        raise ValueError(f"{who}: V = {V} (2 .. {H.TQ_MAX_VOCAB} symbols are on the MI355X path)")
    if not 1 <= K <= H.TQ_MAX_ORDER:
        raise ValueError(f"{who}: max_order = {K} (n-gram orders 1 .. {H.TQ_MAX_ORDER})")
    ids = {}
    for what, v in (("eos", eos), ("trim", trim), ("sep", sep)):
        if v is not None and (isinstance(v, bool) or int(v) != v or not 0 <= int(v) < V):
            raise ValueError(f"{who}: {what} = {v!r} (a token id in [0, {V}), or None)")
        ids[what] = -1 if v is None else int(v)
    if ids["sep"] >= 0 and ids["sep"] == ids["eos"]:
        raise ValueError(f"{who}: sep = eos = {ids['sep']} (the separator must differ from the end marker)")
    return dict(ids, max_order=K)


def _tq_ids(who, what, t, shape, V):
    """contiguous int32 ids of `shape` (a None entry: any size >= 1), every id in [0, V) (V None: unchecked), or ValueError"""
    form = str(shape).replace("None", "T")
    return ck.integers(who, what, t, len(shape), f"integers of shape {form}",
                       [(i, s, s, f"{what} is {{shape}}, not {form}") for i, s in enumerate(shape) if s is not None],
                       inside=None if V is None else (0, V, f"holds ids from {{0}} to {{1}} (token ids lie in [0, {V}))"))


def text_quality(hyp, ref_ids, ref_lengths, hyp_lengths=None, eos=None, trim=None, sep=None, max_order=4):
    """How close the token sequences `hyp` are to the references, pair by pair, in one launch, one wave per pair
    (csrc/text_quality.hip; mmvae_hip.h has the arithmetic).  hyp: floating (N, Th, V) logits, read as fp32 -- the hypothesis
    is their argmax, the first maximum of every step -- or integer (N, Th) ids.  ref_ids integer (N, Tr), ref_lengths integer
    (N,), hyp_lengths integer (N,) or None (Th each); lengths are clamped into [0, T].  eos: a sequence ends before its first
    eos; trim: trailing tokens equal to trim are then dropped; both sides alike, giving h (Lh tokens) and r (Lr).
      token   hyp_len Lh, ref_len Lr, same = #{t < min(Lh, Lr): h_t == r_t}, edit = Levenshtein distance, lcs = longest common
              subsequence, match (N, 4) / total (N, 4): for n = 1 .. max_order the clipped n-gram matches sum_g min(count_h(g),
              count_r(g)) and max(Lh - n + 1, 0); columns n > max_order are 0.
      word    with sep: the same (without `same`) over the words, the maximal runs of tokens != sep; None without.
      pred    (N, Th) the argmax;  nll (N,) float64 = sum_{t < S} (logsumexp(x_t) - x_t[ref_t]), S = min(ref length, Th) =
              nll_steps (N,): before eos / trim, the decoder's objective.  All three None for an ids hypothesis.
    -> {"token": {...}, "word": {...} or None, "pred", "nll", "nll_steps", "max_order"}, int32 tensors on the device.  No
    atomics; a pair's outputs do not depend on the other pairs.  1 <= Th, Tr <= 256, 2 <= V <= 256 (ids form: ids < 256),
    ids in [0, V), sep != eos.  The logits are expected finite and are not scanned (torch's isfinite().all() is five launches over
    the whole tensor): a step that holds a NaN or +inf shows as a NaN in the pair's nll."""
    who = "text_quality"
    if not torch.is_tensor(hyp) or not ((hyp.is_floating_point() and hyp.dim() == 3) or
                                        (not hyp.is_floating_point() and hyp.dim() == 2)):
        raise ValueError(f"{who}: hyp is {ck.said(hyp)}; floating (N, Th, V) logits or integer (N, Th) ids")
    logits = hyp.is_floating_point()
    N, Th = hyp.shape[:2]
    V = hyp.shape[2] if logits else H.TQ_MAX_VOCAB
    if not torch.is_tensor(ref_ids) or ref_ids.dim() != 2:
        raise ValueError(f"{who}: ref_ids is {ck.said(ref_ids)}; integers of shape (N, Tr)")
    Tr = ref_ids.shape[1]
    if not 1 <= N <= H.TQ_MAX_ROWS:
        raise ValueError(f"{who}: {N} pairs (1 .. {H.TQ_MAX_ROWS} a call: one workgroup per pair in one launch)")
    plan = text_quality_plan(Th, Tr, V, eos, trim, sep, max_order)
    ref_ids = _tq_ids(who, "ref_ids", ref_ids, (N, None), V)
    ref_lengths = _tq_ids(who, "ref_lengths", ref_lengths, (N,), None)
    if hyp_lengths is not None:
        hyp_lengths = _tq_ids(who, "hyp_lengths", hyp_lengths, (N,), None)
    hyp = H.f32c(hyp.detach()) if logits else _tq_ids(who, "hyp", hyp, (N, Th), V)
    dev = hyp.device
    if any(t is not None and t.device != dev for t in (ref_ids, ref_lengths, hyp_lengths)):
        raise ValueError(f"{who}: hyp is on {dev}, the references or lengths elsewhere (one device)")
    ck.need_gpu(who, "hyp is", dev)
    K = plan["max_order"]
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    tok, word = i32(N, 13), (i32(N, 12) if plan["sep"] >= 0 else None)
    pred, nll, steps = (i32(N, Th), torch.empty(N, dtype=torch.float64, device=dev), i32(N)) if logits else (None,) * 3
    H.call("mmvae_text_quality", H.ptr(hyp) if logits else None, None if logits else H.ptr(hyp), H.ptr(ref_ids),
           H.ptr(ref_lengths), H.ptr(hyp_lengths), H.ptr(pred), H.ptr(tok), H.ptr(word), H.ptr(nll), H.ptr(steps), N, Th, Tr, V,
           plan["eos"], plan["trim"], plan["sep"], K, H.stream())
    level = lambda o, same: dict(
        {"hyp_len": o[:, 0], "ref_len": o[:, 1], "edit": o[:, 2 + same], "lcs": o[:, 3 + same],
         "match": o[:, 4 + same:8 + same], "total": o[:, 8 + same:12 + same]}, **({"same": o[:, 2]} if same else {}))
    return {"token": level(tok, 1), "word": None if word is None else level(word, 0), "pred": pred, "nll": nll,
            "nll_steps": steps, "max_order": K}


def _tq_level_summary(parts, K, token):
    """the summary of one level from the per-pair integer counts of `parts` (dicts of (n,) / (n, 4) integer tensors)"""
    cat = lambda name: np.concatenate([p[name].detach().cpu().numpy().astype(np.int64) for p in parts])
    hl, rl, edit, lcs, match, total = (cat(k) for k in ("hyp_len", "ref_len", "edit", "lcs", "match", "total"))
    n = len(hl)
    Hs, Rs = int(hl.sum()), int(rl.sum())
    ms, ts = [int(v) for v in match[:, :K].sum(0)], [int(v) for v in total[:, :K].sum(0)]
    bp = lambda h, r: math.exp(1.0 - r / h) if h < r else 1.0
    if Hs == 0 or any(m == 0 for m in ms):
        bleu = 0.0
    else:
        bleu = bp(Hs, Rs) * math.exp(sum(math.log(m / t) for m, t in zip(ms, ts)) / K)
    sent, rouge = [], []
    for i in range(n):
        h, r, l = int(hl[i]), int(rl[i]), int(lcs[i])
        if h == 0 or match[i, 0] == 0:
            sent.append(0.0)
        else:
            logs = [math.log(int(match[i, 0]) / int(total[i, 0]))]
            logs += [math.log((int(match[i, k]) + 1) / (int(total[i, k]) + 1)) for k in range(1, K)]
            sent.append(bp(h, r) * math.exp(sum(logs) / K))
        P, R = (l / h if h else 0.0), (l / r if r else 0.0)
        rouge.append(2.0 * P * R / (P + R) if P + R > 0.0 else 0.0)
    E = int(edit.sum())
    out = {"n": n, "error_rate": E / Rs if Rs else (0.0 if E == 0 else float("inf")),
           "exact": float(np.count_nonzero(edit == 0)) / n, "bleu": bleu,
           "precisions": [m / t if t else 0.0 for m, t in zip(ms, ts)], "sentence_bleu": math.fsum(sent) / n,
           "rouge_l": math.fsum(rouge) / n}
    if token:
        out["accuracy"] = int(cat("same").sum()) / Rs if Rs else 0.0
    return out


def text_quality_summary(parts):
    """The corpus figures of one or several text_quality results (a dict, or a list of them with one max_order), on the host,
    from the INTEGER sums of the per-pair counts.  -> {"token": S, "word": S or None}, S per level:
      n               pairs;
      error_rate      sum edit / sum ref_len: the character / word error rate (CER / WER) where a token is a character
                      (0 / 0 = 0, x / 0 = inf);
      exact           mean(edit == 0);
      accuracy        sum same / sum ref_len (token level only);
      bleu            corpus BLEU (Papineni et al. 2002): brevity penalty times the geometric mean over the orders 1 .. K of
                      sum match_n / sum total_n; brevity penalty exp(1 - sum ref_len / sum hyp_len) when sum hyp_len <
                      sum ref_len; 0 when a sum match_n or sum hyp_len is 0;
      precisions      [sum match_n / sum total_n for n = 1 .. K] (0 for an empty total);
      sentence_bleu   mean over the pairs of the pair's BLEU with Lin & Och's (2004) add-one smoothing of the orders n >= 2,
                      (match_n + 1) / (total_n + 1), order 1 unsmoothed (no unigram match: 0), the pair's own brevity penalty,
                      0 for an empty hypothesis;
      rouge_l         mean over the pairs of F1 = 2 P R / (P + R), P = lcs / hyp_len, R = lcs / ref_len (a zero denominator: 0);
      nll, perplexity, bits_per_token   (token level; None for ids hypotheses) sum nll / sum nll_steps, its exp, and it
                      divided by ln 2; nan when no step was scored."""
    parts = [parts] if isinstance(parts, dict) else list(parts)
    if not parts:
        raise ValueError("text_quality_summary: no parts")
    K = {int(p["max_order"]) for p in parts}
    if len(K) != 1 or len({p["word"] is None for p in parts}) != 1 or len({p["nll"] is None for p in parts}) != 1:
        raise ValueError("text_quality_summary: the parts were scored with different max_order, sep or hypothesis forms")
    K = K.pop()
    token = _tq_level_summary([p["token"] for p in parts], K, True)
    word = None if parts[0]["word"] is None else _tq_level_summary([p["word"] for p in parts], K, False)
    if parts[0]["nll"] is None:
        token.update(nll=None, perplexity=None, bits_per_token=None)
    else:
        steps = sum(int(p["nll_steps"].sum()) for p in parts)
        total = math.fsum(v for p in parts for v in p["nll"].detach().cpu().tolist())
        mean = total / steps if steps else float("nan")
        token.update(nll=mean, perplexity=math.exp(mean), bits_per_token=mean / math.log(2.0))
    return {"token": token, "word": word}
