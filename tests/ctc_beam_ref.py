"""Test helper (not a test): CTC prefix beam search without a language model, restated in
Python doubles from the rules that ``ob_ctc_beam_search`` documents (include/onebit_hip.h;
the reference's decoder is onebit_asr/metrics.py:74-145). fp64 throughout, the log-softmax
included. Besides the hypothesis and its score it reports what a comparison needs to know
about the input: the smallest decision margin, the final beam, and how often a pruned prefix
came back while one of its descendants was live.

Rules: candidates are the ``top_k`` largest logits of a frame in descending order (ties to the
lowest index; all V tokens in index order when ``top_k`` is None or >= V); blank is skipped as
a candidate; per live prefix (best first) with state (p_b, p_nb):
  new[prefix].p_b (+)= lse(p_b, p_nb) + lp[blank]
  c == last(prefix):  new[prefix].p_nb (+)= p_b + lp[c]       (the prefix is not extended)
  otherwise:          new[prefix + (c,)].p_nb (+)= lse(p_b, p_nb) + lp[c]
then the ``beam`` largest lse(p_b, p_nb) stay; exact ties keep dict insertion order.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

NEG_INF = -math.inf


def lse(a: float, b: float) -> float:
    if a == NEG_INF:
        return b
    if b == NEG_INF:
        return a
    hi, lo = (a, b) if a > b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


@dataclass
class BeamResult:
    tokens: List[int]
    score: float
    margin: float  # smallest gap at any decision: prune boundary, top-k boundary, final best
    final_beam: List[List[int]] = field(default_factory=list)
    reentries: int = 0  # frames where a pruned prefix came back under a live descendant
    merges: int = 0  # extensions that landed on a prefix that was itself live


def log_softmax64(row: np.ndarray) -> np.ndarray:
    x = row.astype(np.float64)
    m = x.max()
    return x - (m + math.log(np.exp(x - m).sum()))


def frame_candidates(row: np.ndarray, top_k: Optional[int]) -> Tuple[List[int], float]:
    """Candidate tokens of one fp32 logit row in candidate order, and the gap (in logits, which
    equals the gap in lp) between the last token inside the top-k and the first outside."""
    V = row.shape[0]
    if top_k is None or top_k >= V:
        return list(range(V)), math.inf
    order = np.argsort(-row, kind="stable")[:top_k + 1].tolist()  # stable: lowest index first
    return order[:top_k], float(row[order[top_k - 1]]) - float(row[order[top_k]])


def beam_search(logits: np.ndarray, beam: int = 10, blank: int = 3,
                top_k: Optional[int] = 20) -> BeamResult:
    """logits [L, V] fp32: the valid frames of one utterance."""
    L = logits.shape[0]
    beams: Dict[Tuple[int, ...], Tuple[float, float]] = {(): (0.0, NEG_INF)}
    margin = math.inf
    ever_live = {()}
    reentries = merges = 0
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
                    o_b, o_nb = new.get(ext, (NEG_INF, NEG_INF))
                    new[ext] = (o_b, lse(o_nb, tot + lp_c))
        ranked = sorted(new.items(), key=lambda kv: lse(*kv[1]), reverse=True)  # stable
        if len(ranked) > beam:
            margin = min(margin, lse(*ranked[beam - 1][1]) - lse(*ranked[beam][1]))
        kept = dict(ranked[:beam])
        live = set(beams) | set(kept)
        back = [p for p in kept if p not in beams and p in ever_live]
        if any(len(q) > len(p) and q[:len(p)] == p for p in back for q in live):
            reentries += 1
        ever_live.update(kept)
        beams = kept
    ranked = sorted(beams.items(), key=lambda kv: lse(*kv[1]), reverse=True)
    if len(ranked) > 1:
        margin = min(margin, lse(*ranked[0][1]) - lse(*ranked[1][1]))
    return BeamResult(tokens=list(ranked[0][0]), score=lse(*ranked[0][1]), margin=margin,
                      final_beam=[list(p) for p, _ in ranked], reentries=reentries,
                      merges=merges)


def beam_search_fresh_ids(logits: np.ndarray, beam: int = 10, blank: int = 3,
                          top_k: Optional[int] = 20) -> BeamResult:
    """The mistake a device search can make, kept here so that a test can show its inputs tell
    the two apart: every prefix gets a NEW id when it is created, and an extension (i, c) lands
    on a live entry m only when m's recorded parent id is i's id. A prefix that was pruned and
    is built again then has another id than the one its still-live children remember, their
    merge is missed, and one tuple is carried as two entries. Same arithmetic as beam_search
    otherwise; ``merges`` counts the merges that were missed (0: the input cannot tell)."""
    L = logits.shape[0]
    # entry: [id, parent id, tokens, p_b, p_nb]
    live = [[0, -1, (), 0.0, NEG_INF]]
    next_id = 1
    missed = 0
    for t in range(L):
        lp = log_softmax64(logits[t])
        cands, _ = frame_candidates(logits[t], top_k)
        lp_blank = float(lp[blank])
        new: Dict[object, list] = {}  # key: a live entry's id, or (parent id, token) when new
        tuples = {e[2]: e for e in live}
        for eid, _par, toks, p_b, p_nb in live:
            tot = lse(p_b, p_nb)
            cur = new.setdefault(eid, [None, NEG_INF, NEG_INF])
            cur[1] = lse(cur[1], tot + lp_blank)
            last = toks[-1] if toks else None
            for c in cands:
                if c == blank:
                    continue
                lp_c = float(lp[c])
                if c == last:
                    cur = new[eid]
                    cur[2] = lse(cur[2], p_b + lp_c)
                    continue
                child = tuples.get(toks + (c,))
                if child is not None and child[1] == eid:
                    key = child[0]
                else:
                    key = (eid, c)
                    missed += child is not None
                cur = new.setdefault(key, [(eid, toks + (c,)), NEG_INF, NEG_INF])
                cur[2] = lse(cur[2], tot + lp_c)
        by_id = {e[0]: e for e in live}
        ranked = sorted(new.items(), key=lambda kv: lse(kv[1][1], kv[1][2]), reverse=True)[:beam]
        live = []
        for key, (made, p_b, p_nb) in ranked:
            if isinstance(key, tuple):
                live.append([next_id, made[0], made[1], p_b, p_nb])
                next_id += 1
            else:
                old = by_id[key]
                live.append([old[0], old[1], old[2], p_b, p_nb])
    best = max(live, key=lambda e: lse(e[3], e[4]))
    return BeamResult(tokens=list(best[2]), score=lse(best[3], best[4]), margin=math.nan,
                      final_beam=[list(e[2]) for e in live], merges=missed)


def beam_search_batch(logits: np.ndarray, lens: Sequence[int], beam: int = 10, blank: int = 3,
                      top_k: Optional[int] = 20) -> List[BeamResult]:
    T = logits.shape[1]
    return [beam_search(logits[b, :min(max(int(n), 0), T)], beam, blank, top_k)
            for b, n in enumerate(lens)]


def ctc_like_logits(seed: int, B: int, T: int, V: int, blank: int = 3, n_tokens: int = 6,
                    peak: float = 3.0) -> np.ndarray:
    """Unit normal noise plus a +peak per frame: on blank half the time, otherwise on one of
    about ``n_tokens`` tokens fixed per seed, so that prefixes compete, merge and come back."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    pool = np.array([v for v in range(V) if v != blank])
    toks = rng.choice(pool, size=min(n_tokens, pool.size), replace=False)
    is_blank = rng.random((B, T)) < 0.5
    pick = toks[rng.integers(0, toks.size, size=(B, T))]
    peak_at = np.where(is_blank, blank, pick)
    np.add.at(x, (np.arange(B)[:, None], np.arange(T)[None, :], peak_at), np.float32(peak))
    return x


def ragged_lens(seed: int, B: int, T: int) -> np.ndarray:
    """Ragged valid lengths that include T (first) and 0 (last, when B > 1)."""
    rng = np.random.default_rng(seed + 7919)
    lens = rng.integers(0, T + 1, size=B).astype(np.int64)
    lens[0] = T
    if B > 1:
        lens[-1] = 0
    return lens
