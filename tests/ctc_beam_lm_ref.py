"""Test helper (not a test): the CTC prefix beam search of tests/ctc_beam_ref.py with an n-gram LM
inside the search, restated in Python doubles from the rule that ``ob_ctc_beam_search_lm``
documents (include/onebit_hip.h). The candidates, the three transitions, the merges and the dict
insertion order are ``ctc_beam_ref.beam_search``'s; what changes is what a frame's pruning compares.

Every prefix y carries lm(y) = sum_j score([bos] + y[:j], y[j]) (``ngram_ref.RefLM``'s rule, a
float64 sum in ascending position, 0 for the empty prefix; a function of the tuple alone, so a
merge keeps one value). After a frame the ``beam`` largest
    key(y) = (lse(p_b, p_nb) + lm_weight * lm(y)) + ins_bonus * len(y)
stay, every operation a rounded Python float operation; exact ties keep dict insertion order.
After the last frame lm_fin(y) = lm(y) + score([bos] + y, eos), total(y) = (ctc(y) + lm_weight *
lm_fin(y)) + ins_bonus * len(y), and the final beam is ordered by total descending (stable).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ctc_beam_ref import NEG_INF, frame_candidates, log_softmax64, lse
from ngram_ref import EOS, RefLM


def fuse(ctc: float, lw: float, lm: float, bonus: float, n: int) -> float:
    """(ctc + lw * lm) + bonus * n, each of the four operations rounded on its own."""
    pl = lw * lm
    base = ctc + pl
    pn = bonus * float(n)
    return base + pn


@dataclass
class LMBeamResult:
    beam: List[Tuple[List[int], float, float, float]]  # (tokens, ctc, lm_fin, total), best first
    margin: float  # smallest gap at any decision: top-k boundary, prune boundary, final best
    gap: float     # smallest gap between adjacent final totals (inf with fewer than two entries)
    merges: int = 0
    final_beam: List[List[int]] = field(default_factory=list)

    @property
    def tokens(self) -> List[int]:
        return self.beam[0][0]


def lm_beam_search(logits: np.ndarray, lm: RefLM, lm_weight: float, ins_bonus: float = 0.0,
                   beam: int = 10, blank: int = 3, top_k: Optional[int] = 20) -> LMBeamResult:
    """logits [L, V] fp32: the valid frames of one utterance."""
    L = logits.shape[0]
    beams: Dict[Tuple[int, ...], Tuple[float, float]] = {(): (0.0, NEG_INF)}
    lmv: Dict[Tuple[int, ...], float] = {(): 0.0}
    margin = math.inf
    merges = 0

    def key(kv):
        p, (p_b, p_nb) = kv
        return fuse(lse(p_b, p_nb), lm_weight, lmv[p], ins_bonus, len(p))

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
                    if ext in beams:
                        merges += 1
                    if ext not in lmv:
                        lmv[ext] = lmv[prefix] + lm.score(list(prefix), c)
                    o_b, o_nb = new.get(ext, (NEG_INF, NEG_INF))
                    new[ext] = (o_b, lse(o_nb, tot + lp_c))
        ranked = sorted(new.items(), key=key, reverse=True)  # stable: insertion order on ties
        if len(ranked) > beam:
            margin = min(margin, key(ranked[beam - 1]) - key(ranked[beam]))
        beams = dict(ranked[:beam])
        lmv = {p: lmv[p] for p in beams}
    final = []
    for p, (p_b, p_nb) in beams.items():
        ctc = lse(p_b, p_nb)
        lm_fin = lmv[p] + lm.score(list(p), EOS)
        final.append((list(p), ctc, lm_fin, fuse(ctc, lm_weight, lm_fin, ins_bonus, len(p))))
    final.sort(key=lambda e: e[3], reverse=True)  # stable: the beam's order on ties
    gaps = [a[3] - b[3] for a, b in zip(final, final[1:])]
    if gaps:
        margin = min(margin, gaps[0])
    return LMBeamResult(beam=final, margin=margin, gap=min(gaps, default=math.inf), merges=merges,
                        final_beam=[e[0] for e in final])


def lm_beam_search_batch(logits: np.ndarray, lens: Sequence[int], lm: RefLM, lm_weight: float,
                         ins_bonus: float = 0.0, beam: int = 10, blank: int = 3,
                         top_k: Optional[int] = 20) -> List[LMBeamResult]:
    T = logits.shape[1]
    return [lm_beam_search(logits[b, :min(max(int(n), 0), T)], lm, lm_weight, ins_bonus, beam,
                           blank, top_k) for b, n in enumerate(lens)]
