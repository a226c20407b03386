"""Test helper (not a test): the oracle of two-pass decoding (CTC n-best + attention rescoring),
numpy / torch float64 on the CPU.

* ``nbest_search``: the search of ``ctc_beam_ref.beam_search`` restated so that it returns every
  entry of the final beam with its score, best first (total descending, exact ties in dict
  insertion order), and the smallest decision margin -- which here includes the gap between
  every pair of neighbours in the final ranking, because their order is part of the result.
* ``decoder_scores``: a deep copy of the product model on the CPU in ``.double()`` (CPU tensors
  run torch's stock decoder modules), ``decode_logits`` -> ``log_softmax`` -> gather.
* ``prepare`` / ``select`` / ``seq_logprob``: plain Python / numpy float64.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ctc_beam_ref import NEG_INF, frame_candidates, log_softmax64, lse

PAD, BOS, EOS, BLANK = 0, 1, 2, 3


@dataclass
class NBestResult:
    hyps: List[List[int]]   # the final beam, best first
    scores: List[float]     # lse(p_b, p_nb) of each
    margin: float           # smallest gap at any decision, the final ranking's included


def nbest_search(logits: np.ndarray, beam: int = 10, blank: int = BLANK,
                 top_k: Optional[int] = 20) -> NBestResult:
    """logits [L, V] fp32: the valid frames of one utterance."""
    L = logits.shape[0]
    beams: Dict[Tuple[int, ...], Tuple[float, float]] = {(): (0.0, NEG_INF)}
    margin = math.inf
    for t in range(L):
        lp = log_softmax64(logits[t])
        cands, gap = frame_candidates(logits[t], top_k)
        margin = min(margin, gap)
        lp_blank = float(lp[blank])
        new: Dict[Tuple[int, ...], Tuple[float, float]] = {}
        for prefix, (p_b, p_nb) in beams.items():
            tot = lse(p_b, p_nb)
            o_b, o_nb = new.get(prefix, (NEG_INF, NEG_INF))
            new[prefix] = (lse(o_b, tot + lp_blank), o_nb)
            last = prefix[-1] if prefix else None
            for c in cands:
                if c == blank:
                    continue
                lp_c = float(lp[c])
                if c == last:
                    o_b, o_nb = new[prefix]
                    new[prefix] = (o_b, lse(o_nb, p_b + lp_c))
                else:
                    ext = prefix + (c,)
                    o_b, o_nb = new.get(ext, (NEG_INF, NEG_INF))
                    new[ext] = (o_b, lse(o_nb, tot + lp_c))
        ranked = sorted(new.items(), key=lambda kv: lse(*kv[1]), reverse=True)  # stable
        if len(ranked) > beam:
            margin = min(margin, lse(*ranked[beam - 1][1]) - lse(*ranked[beam][1]))
        beams = dict(ranked[:beam])
    ranked = sorted(beams.items(), key=lambda kv: lse(*kv[1]), reverse=True)
    scores = [lse(*v) for _, v in ranked]
    for a, b in zip(scores, scores[1:]):
        margin = min(margin, a - b)
    return NBestResult([list(p) for p, _ in ranked], scores, margin)


def nbest_search_batch(logits: np.ndarray, lens: Sequence[int], beam: int = 10,
                       blank: int = BLANK, top_k: Optional[int] = 20) -> List[NBestResult]:
    T = logits.shape[1]
    return [nbest_search(logits[b, :min(max(int(n), 0), T)], beam, blank, top_k)
            for b, n in enumerate(lens)]


def prepare(hyps: Sequence[Sequence[Sequence[int]]], n_slots: int, Lc: int, bos: int = BOS,
            eos: int = EOS, pad: int = PAD):
    """hyps[b] = the live hypotheses of utterance b (token lists), n_slots = N >= len(hyps[b]).
    -> (tgt_inp [B*N][Lc+1], target, tgt_pad, ok [B]) as nested lists, by the rules of
    ``ob_rescore_prepare``."""
    tgt_inp, target, tgt_pad, ok = [], [], [], []
    for utt in hyps:
        fits = all(len(y) <= Lc for y in utt)
        ok.append(1 if fits else 0)
        for k in range(n_slots):
            live = fits and k < len(utt)
            y = list(utt[k]) if live else []
            n = len(y)
            tgt_inp.append([bos] + y + [pad] * (Lc - n))
            target.append((y + [eos] + [-1] * (Lc - n)) if live else [-1] * (Lc + 1))
            tgt_pad.append([0] * (n + 1) + [1] * (Lc - n))
    return tgt_inp, target, tgt_pad, ok


def seq_logprob(hidden: np.ndarray, weight: np.ndarray, bias: Optional[np.ndarray],
                target: Sequence[int]) -> Tuple[np.ndarray, float]:
    """float64 lp [R] (0 for target -1) and max |logit|."""
    z = hidden.astype(np.float64) @ weight.astype(np.float64).T
    if bias is not None:
        z = z + bias.astype(np.float64)
    m = z.max(axis=1, keepdims=True) if z.size else z
    lsm = z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))) if z.size else z
    out = np.zeros(len(target), np.float64)
    for r, t in enumerate(target):
        if t >= 0:
            out[r] = lsm[r, t]
    return out, float(np.abs(z).max()) if z.size else 0.0


def select(lp: Sequence[Sequence[float]], hyps: Sequence[Sequence[Sequence[int]]],
           ctc: Sequence[Sequence[float]], ok: Sequence[int], n_slots: int, ctc_weight: float):
    """lp[b*N + k][j]; -> per utterance (best_k, tokens, att [N], total [N], rescored) by the
    rules of ``ob_rescore_select``."""
    res = []
    for b, utt in enumerate(hyps):
        att = [0.0] * n_slots
        total = [NEG_INF] * n_slots
        if ok[b]:
            for k, y in enumerate(utt):
                a = 0.0
                for j in range(len(y) + 1):
                    a += float(lp[b * n_slots + k][j])
                att[k] = a
                total[k] = a + ctc_weight * float(ctc[b][k])
        k_best = 0
        if ok[b]:
            for k in range(1, len(utt)):
                if total[k] > total[k_best]:  # strict: ties stay with the smaller k
                    k_best = k
        res.append((k_best, list(utt[k_best]), att, total, bool(ok[b])))
    return res


def double_model(model):
    """A CPU float64 deep copy of the product model, in eval mode."""
    return copy.deepcopy(model).cpu().double().eval()


def decoder_scores(model64, enc: np.ndarray, mask: np.ndarray,
                   hyps: Sequence[Sequence[Sequence[int]]], bos: int = BOS, eos: int = EOS,
                   pad: int = PAD) -> List[List[float]]:
    """att[b][k] = sum_j log_softmax(decode_logits)[j, target_j] of hypothesis k of utterance b
    under teacher forcing, float64 (each utterance at its own longest hypothesis)."""
    import torch

    out = []
    with torch.no_grad():
        for b, utt in enumerate(hyps):
            Lc = max(len(y) for y in utt)
            inp, tgt, padm, _ = prepare([utt], len(utt), Lc, bos, eos, pad)
            n = len(utt)
            e = torch.from_numpy(enc[b:b + 1].astype(np.float64)).repeat(n, 1, 1)
            m = torch.from_numpy(np.asarray(mask[b:b + 1])).repeat(n, 1)
            z = model64.decode_logits(e, m, torch.tensor(inp, dtype=torch.long),
                                      torch.tensor(padm, dtype=torch.bool))
            lsm = torch.log_softmax(z, dim=-1)
            row = []
            for k in range(n):
                row.append(sum(float(lsm[k, j, tgt[k][j]]) for j in range(len(utt[k]) + 1)))
            out.append(row)
    return out
