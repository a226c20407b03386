"""Test helper (not a test): the float64 oracle of CTC forced alignment
(``onebit_asr.align.ctc_forced_align``, csrc/align.hip). Numpy only.

``viterbi(x, target, blank)``: x [T, V] the float64 log-softmax of the CTC logits of the T valid
frames. Extended labels l' = blank, target_0, blank, ..., blank (2 L + 1 states); state s may be
entered from s, s - 1 and, for a token state whose token differs from the previous token's,
s - 2. v_t(s) = max(allowed predecessors) + x[t][l'(s)]. Ties: stay wins over s - 1, which wins
over s - 2; at the last frame the final token state wins against the trailing blank.

``brute_force(x, blank, max_len)``: the best score of every target of up to ``max_len`` tokens by
enumerating all V ** T frame labellings.
"""
from __future__ import annotations

import itertools
import math
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np

from joint_ref import log_softmax64  # noqa: F401  (re-exported for the tests)

NEG_INF = -math.inf


class Viterbi(NamedTuple):
    score: float                    # -inf: no alignment
    path: List[int]                 # [T] token id per frame (blank for a blank frame), -1 if none
    spans: List[Tuple[int, int]]    # [L] (first frame, last frame + 1), (-1, -1) if none
    tok_scores: List[float]         # [L] sum of x[t][token] over the span, 0 if none
    margin: float                   # smallest best-to-second-best gap over the path's decisions


def _none(T: int, L: int) -> Viterbi:
    return Viterbi(NEG_INF, [-1] * T, [(-1, -1)] * L, [0.0] * L, math.inf)


def _gap(best: float, others: Sequence[float]) -> float:
    rest = [o for o in others if o != NEG_INF]
    return best - max(rest) if rest else math.inf


def viterbi(x: np.ndarray, target: Sequence[int], blank: int) -> Viterbi:
    x = np.asarray(x, np.float64)
    T, V = x.shape
    target = [int(c) for c in target]
    L = len(target)
    if any(c < 0 or c >= V or c == blank for c in target) or (T == 0 and L > 0):
        return _none(T, L)
    if T == 0:
        return Viterbi(0.0, [], [], [], math.inf)
    NS = 2 * L + 1
    lab = [target[s >> 1] if s & 1 else blank for s in range(NS)]
    v = [NEG_INF] * NS
    v[0] = float(x[0][blank])
    if NS > 1:
        v[1] = float(x[0][lab[1]])
    back = np.zeros((T, NS), np.int64)
    gap = np.full((T, NS), math.inf)
    for t in range(1, T):
        new = [NEG_INF] * NS
        for s in range(NS):
            cands = [v[s]]
            if s >= 1:
                cands.append(v[s - 1])
            if s >= 3 and s & 1 and lab[s] != lab[s - 2]:
                cands.append(v[s - 2])
            d = 0
            for k in range(1, len(cands)):
                if cands[k] > cands[d]:      # strict: the earlier candidate keeps a tie
                    d = k
            if cands[d] != NEG_INF:
                gap[t][s] = _gap(cands[d], cands[:d] + cands[d + 1:])
            back[t][s] = d
            new[s] = cands[d] + float(x[t][lab[s]])
        v = new
    s, score, margin = NS - 1, v[NS - 1], math.inf
    if NS >= 2:
        if v[NS - 2] >= score:               # the final token wins a tie against the blank
            s, score = NS - 2, v[NS - 2]
        if score != NEG_INF:
            margin = _gap(score, [v[NS - 1] if s == NS - 2 else v[NS - 2]])
    if score == NEG_INF:
        return _none(T, L)
    states = [0] * T
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t > 0:
            margin = min(margin, float(gap[t][s]))
            s -= int(back[t][s])
    assert s in (0, 1)
    path = [lab[q] for q in states]
    spans, toks = [], []
    for u in range(L):
        fr = [t for t, q in enumerate(states) if q == 2 * u + 1]
        assert fr == list(range(fr[0], fr[-1] + 1))
        spans.append((fr[0], fr[-1] + 1))
        acc = 0.0
        for t in fr:
            acc += float(x[t][target[u]])
        toks.append(acc)
    return Viterbi(float(score), path, spans, toks, margin)


def collapse(path: Sequence[int], blank: int) -> List[int]:
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def brute_force(x: np.ndarray, blank: int) -> Dict[Tuple[int, ...], float]:
    """{target: the best alignment score} over all V ** T frame labellings; a target that is
    absent has no alignment."""
    T, V = x.shape
    best: Dict[Tuple[int, ...], float] = {}
    for p in itertools.product(range(V), repeat=T):
        lp = float(sum(x[t][c] for t, c in enumerate(p)))
        key = tuple(collapse(p, blank))
        if lp > best.get(key, NEG_INF):
            best[key] = lp
    return best
