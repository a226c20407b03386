"""Test helper (not a test): the oracle of the phrase-list contextual biasing (onebit_asr/bias.py,
csrc/bias.hip, the biased searches of csrc/beam.hip and csrc/attdec.hip), restated on Python tuples
and dicts from the rule that include/onebit_hip.h documents.

* ``RefBias``: the phrases as a dict of tuples. A node is a token path (a tuple), the root ``()``.
  With val(n, b) = float32(float64(n) * float64(b)):

      commit(p) = max val(len q, b_q) over phrases q that are a prefix of p (q == p included), or 0
      phi(p)    = max(commit(p), max val(len p, b_q) over phrases q that p is a prefix of)
      fail(p)   = the longest proper suffix of p that is a node
      step:  u = state
             loop:  child(u, w) exists -> t = it, stop
                    commit(u) > 0      -> kept += commit(u); t = child(root, w) or root, stop
                    u == root          -> t = root, stop
                    u = fail(u)
             t != root and t has no children -> kept += commit(t); t = root
      bias(y) = kept + phi(state),  bias_fin(y) = kept + commit(state)

  Nothing is precomputed beyond the phrase dict and the node set: every quantity is evaluated from
  its definition, so the oracle shares no table and no numbering with the library.
* ``biased_beam_search``: ``ctc_beam_lm_ref.lm_beam_search`` with the bias term in the key and the
  total (``lm=None``: no LM, lm(y) = lm_fin = 0).
* ``biased_search``: ``ngram_ref.fused_search`` with the bias term (``lm=None``: Lm = 0).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from attdec_ref import CARRIED, DEAD, SPECIAL, length_norm, rank
from ctc_beam_lm_ref import fuse
from ctc_beam_ref import NEG_INF, frame_candidates, log_softmax64, lse
from joint_ref import combine, eos_score, extend, root, top_candidates
from ngram_ref import EOS


def val(n: int, b: float) -> float:
    return float(np.float32(np.float64(n) * np.float64(np.float32(b))))


class RefBias:
    def __init__(self, phrases: Sequence, boost: float = 1.0):
        self.phrases: Dict[Tuple[int, ...], float] = {}
        for p in phrases:
            if len(p) == 2 and isinstance(p[0], (tuple, list)):
                ids, b = tuple(int(t) for t in p[0]), float(np.float32(p[1]))
            else:
                ids, b = tuple(int(t) for t in p), float(np.float32(boost))
            self.phrases[ids] = max(self.phrases.get(ids, 0.0), b)   # a duplicate: the larger
        self.nodes = {q[:n] for q in self.phrases for n in range(len(q) + 1)} | {()}

    def commit(self, p: Tuple[int, ...]) -> float:
        return max([val(len(q), b) for q, b in self.phrases.items() if p[:len(q)] == q] or [0.0])

    def phi(self, p: Tuple[int, ...]) -> float:
        over = [val(len(p), b) for q, b in self.phrases.items() if q[:len(p)] == p]
        return max([self.commit(p)] + (over if p else []))

    def fail(self, p: Tuple[int, ...]) -> Tuple[int, ...]:
        for start in range(1, len(p) + 1):
            if p[start:] in self.nodes:
                return p[start:]
        return ()

    def has_children(self, p: Tuple[int, ...]) -> bool:
        return any(len(q) > len(p) and q[:len(p)] == p for q in self.phrases)

    def step(self, state: Tuple[int, ...], kept: float, w: int, tags: Optional[set] = None):
        """-> (state, kept) after token w; ``tags`` collects the branches taken."""
        tags = set() if tags is None else tags
        u = state
        lookups = 0
        while True:
            lookups += 1
            if u + (w,) in self.nodes:
                t = u + (w,)
                tags.add("edge" if u == state else "edge_after_fail")
                break
            if self.commit(u) > 0:
                kept += self.commit(u)
                lookups += 1
                t = (w,) if (w,) in self.nodes else ()
                tags.add("commit" if u == state else "commit_on_fail_path")
                tags.add("restart_hit" if t else "restart_miss")
                break
            if u == ():
                t = ()
                tags.add("root_miss")
                break
            u = self.fail(u)
        assert lookups <= 17
        if t != () and not self.has_children(t):
            kept += self.commit(t)
            t = ()
            tags.add("leaf")
        return t, kept

    def walk(self, tokens: Sequence[int], tags: Optional[set] = None):
        """-> (state, kept, bias, bias_fin) of a token sequence."""
        state, kept = (), 0.0
        for w in tokens:
            state, kept = self.step(state, kept, int(w), tags)
        return state, kept, kept + self.phi(state), kept + self.commit(state)

    def bias(self, tokens: Sequence[int]) -> float:
        return self.walk(tokens)[2]

    def bias_fin(self, tokens: Sequence[int]) -> float:
        return self.walk(tokens)[3]


def node_numbers(ref: RefBias) -> Dict[Tuple[int, ...], int]:
    """The contract's numbering: breadth-first by depth, within a depth by (parent number, token)."""
    num = {(): 0}
    depth = 1
    while True:
        level = [p for p in ref.nodes if len(p) == depth]
        if not level:
            return num
        for p in sorted(level, key=lambda p: (num[p[:-1]], p[-1])):
            num[p] = len(num)
        depth += 1


# ------------------------------------------------------------------------------------------
# the biased CTC prefix beam search
# ------------------------------------------------------------------------------------------
def bfuse(ctc: float, lw: float, lm: float, bonus: float, n: int, bw: float, bv: float) -> float:
    """((ctc + lw * lm) + bonus * n) + bw * bias, every operation rounded on its own."""
    return fuse(ctc, lw, lm, bonus, n) + bw * bv


@dataclass
class BiasBeamResult:
    beam: List[Tuple[List[int], float, float, float, float]]  # (tokens, ctc, lm_fin, bias_fin, total)
    margin: float
    gap: float
    merges: int = 0
    final_beam: List[List[int]] = field(default_factory=list)

    @property
    def tokens(self) -> List[int]:
        return self.beam[0][0]


def biased_beam_search(logits: np.ndarray, bias: RefBias, bias_weight: float, lm=None,
                       lm_weight: float = 0.0, ins_bonus: float = 0.0, beam: int = 10,
                       blank: int = 3, top_k: Optional[int] = 20) -> BiasBeamResult:
    """logits [L, V] fp32: the valid frames of one utterance."""
    L = logits.shape[0]
    beams: Dict[Tuple[int, ...], Tuple[float, float]] = {(): (0.0, NEG_INF)}
    lmv: Dict[Tuple[int, ...], float] = {(): 0.0}
    bst: Dict[Tuple[int, ...], Tuple[Tuple[int, ...], float]] = {(): ((), 0.0)}
    margin = math.inf
    merges = 0

    def running(p):
        state, kept = bst[p]
        return kept + bias.phi(state)

    def key(kv):
        p, (p_b, p_nb) = kv
        return bfuse(lse(p_b, p_nb), lm_weight, lmv[p], ins_bonus, len(p), bias_weight, running(p))

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
                        lmv[ext] = lmv[prefix] + lm.score(list(prefix), c) if lm is not None \
                            else 0.0
                    if ext not in bst:
                        bst[ext] = bias.step(*bst[prefix], c)
                    o_b, o_nb = new.get(ext, (NEG_INF, NEG_INF))
                    new[ext] = (o_b, lse(o_nb, tot + lp_c))
        ranked = sorted(new.items(), key=key, reverse=True)  # stable: insertion order on ties
        if len(ranked) > beam:
            margin = min(margin, key(ranked[beam - 1]) - key(ranked[beam]))
        beams = dict(ranked[:beam])
        lmv = {p: lmv[p] for p in beams}
        bst = {p: bst[p] for p in beams}
    final = []
    for p, (p_b, p_nb) in beams.items():
        ctc = lse(p_b, p_nb)
        lm_fin = lmv[p] + lm.score(list(p), EOS) if lm is not None else 0.0
        state, kept = bst[p]
        b_fin = kept + bias.commit(state)
        final.append((list(p), ctc, lm_fin, b_fin,
                      bfuse(ctc, lm_weight, lm_fin, ins_bonus, len(p), bias_weight, b_fin)))
    final.sort(key=lambda e: e[4], reverse=True)  # stable: the beam's order on ties
    gaps = [a[4] - b[4] for a, b in zip(final, final[1:])]
    if gaps:
        margin = min(margin, gaps[0])
    return BiasBeamResult(beam=final, margin=margin, gap=min(gaps, default=math.inf),
                          merges=merges, final_beam=[e[0] for e in final])


def biased_beam_search_batch(logits: np.ndarray, lens: Sequence[int], bias: RefBias,
                             bias_weight: float, lm=None, lm_weight: float = 0.0,
                             ins_bonus: float = 0.0, beam: int = 10, blank: int = 3,
                             top_k: Optional[int] = 20) -> List[BiasBeamResult]:
    T = logits.shape[1]
    return [biased_beam_search(logits[b, :min(max(int(n), 0), T)], bias, bias_weight, lm, lm_weight,
                               ins_bonus, beam, blank, top_k) for b, n in enumerate(lens)]


# ------------------------------------------------------------------------------------------
# the biased attention / joint search
# ------------------------------------------------------------------------------------------
@dataclass
class BSlot:
    toks: List[int]
    A: float
    C: float
    Lm: float
    Bi: float
    S: float
    n: int
    fin: bool
    gn: Optional[List[float]] = None
    gb: Optional[List[float]] = None

    @property
    def score(self):
        return self.S


@dataclass
class BiasedResult:
    hyps: List[List[int]]
    scores: List[float]
    att: List[float]
    ctc: List[float]
    lm: List[float]
    bias: List[float]
    finished: List[bool]
    margin: float
    dropped: int
    trace: List[List[Tuple[int, int, float]]] = field(default_factory=list)
    history: List[List[Optional[BSlot]]] = field(default_factory=list)


def bscore(w: float, lw: float, bw: float, a: float, c: float, lm: float, bv: float) -> float:
    """(((1 - w) * A + w * C) + lw * Lm) + bw * Bi, every operation rounded."""
    return (combine(w, a, c) + lw * lm) + bw * bv


def biased_search(logp: Callable[[List[List[int]]], Sequence[np.ndarray]], x: np.ndarray,
                  bias: RefBias, bw: float, N: int, K: int, L: int, w: float, lm=None,
                  lw: float = 0.0, alpha: float = 0.0, special: Optional[Dict[str, int]] = None,
                  alive: bool = True, cscore=None) -> BiasedResult:
    """``ngram_ref.fused_search`` with the bias term: a candidate's Bi' is bias(y . c), the running
    value (an absolute value, not an increment), bias_fin(y) for eos; ``lm=None``: Lm' = 0."""
    ids = dict(SPECIAL, **(special or {}))
    banned = {ids["pad"], ids["bos"], ids["blank"]}
    norm = length_norm(L, alpha)
    first = None
    if alive:
        gn, gb = root(x, ids["blank"]) if w > 0 and cscore is None else (None, None)
        first = BSlot([], 0.0, 0.0, 0.0, 0.0, 0.0, 0, False, gn, gb)
    slots: List[Optional[BSlot]] = [first] + [None] * (N - 1)
    margin, dropped, trace = math.inf, 0, []
    history = [slots]
    for _ in range(L):
        live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
        lps = dict(zip(live, logp([slots[k].toks for k in live]))) if live else {}
        cands = []
        for k, s in enumerate(slots):
            if s is None:
                continue
            if s.fin:
                cands.append((s.S / norm[s.n], k, CARRIED, s.S, s.A, s.C, s.Lm, s.Bi, s.n, None,
                              None))
                continue
            lp = np.asarray(lps[k], np.float64)
            for v in map(int, top_candidates(lp, banned, K)):
                a = s.A + float(lp[v])
                gn = gb = None
                if cscore is not None:
                    c = cscore(s.toks, v)
                elif w == 0:
                    c = 0.0
                elif v == ids["eos"]:
                    c = eos_score(s.gn, s.gb)
                else:
                    gn, gb, c = extend(x, ids["blank"], s.toks, s.gn, s.gb, v)
                if w > 0 and c == NEG_INF:
                    dropped += 1
                    continue
                l_ = s.Lm + lm.score(s.toks, v) if lm is not None else 0.0
                bv = bias.bias_fin(s.toks) if v == ids["eos"] else bias.bias(s.toks + [v])
                sc = bscore(w, lw, bw, a, c, l_, bv)
                cands.append((sc / norm[s.n + 1], k, v, sc, a, c, l_, bv, s.n + 1, gn, gb))
        ranked = rank(cands)
        if len(ranked) > N:
            margin = min(margin, ranked[N - 1][0] - ranked[N][0])
        new: List[Optional[BSlot]] = []
        row = []
        for key, k, v, sc, a, c, l_, bv, n, gn, gb in ranked[:N]:
            s = slots[k]
            if v == CARRIED or v == ids["eos"]:
                new.append(BSlot(list(s.toks), a, c, l_, bv, sc, n, True))
            else:
                new.append(BSlot(s.toks + [v], a, c, l_, bv, sc, n, False, gn, gb))
            row.append((k, v, sc))
        while len(new) < N:
            new.append(None)
            row.append((-1, DEAD, NEG_INF))
        slots = new
        trace.append(row)
        history.append(slots)
    alive_slots = [s for s in slots if s is not None]
    keys = [s.S / norm[s.n] for s in alive_slots]
    for a, b in zip(keys, keys[1:]):
        margin = min(margin, a - b)
    return BiasedResult([s.toks for s in alive_slots], [s.S for s in alive_slots],
                        [s.A for s in alive_slots], [s.C for s in alive_slots],
                        [s.Lm for s in alive_slots], [s.Bi for s in alive_slots],
                        [s.fin for s in alive_slots], margin, dropped, trace, history)
