"""Test helper (not a test): the float64 oracle of the attention-decoder beam search
(``decoder="attention"``, onebit_asr/attdec.py).

* ``beam_search``: the bookkeeping alone, a function of a callable ``logp(prefixes)`` that returns
  one float64 log-probability vector [V] per prefix (all live prefixes of a step have the same
  length). It returns the slots after ``L`` steps, best key first, the back-pointer trace and
  the smallest decision margin: the key gap between the last kept and the first dropped
  candidate of every step, and the gaps inside the final ranking.
* ``model_logp``: ``rescore_ref.double_model(model).decode_logits`` WITHOUT a cache, on each
  growing prefix, ``log_softmax`` of the last position.

Rules (the device's): before step 0 only slot 0 is live (score 0, empty prefix). A live,
unfinished slot r contributes (r, v) for every v outside {pad, bos, blank} with score
``s_r + lp_r[v]``; a finished slot contributes itself, unchanged; dead slots nothing. Key =
score / norm[n], norm[n] = max(n, 1) ** alpha, n = emitted tokens with eos counted. The N
largest keys are kept in key order, ties to the smaller slot, then the smaller token. A selected
eos finishes the slot and is not part of the hypothesis.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

SPECIAL = {"pad": 0, "bos": 1, "eos": 2, "blank": 3}
NEG_INF = -math.inf
CARRIED, DEAD = -1, -2  # trace_token of a finished slot carried over / of a dead slot


def length_norm(L: int, alpha: float) -> List[float]:
    return [float(max(n, 1)) ** float(alpha) for n in range(L + 1)]


@dataclass
class Slot:
    toks: List[int]
    score: float
    n: int            # emitted tokens, eos counted
    fin: bool


@dataclass
class AttResult:
    hyps: List[List[int]]            # live slots, best key first (eos not stored)
    scores: List[float]
    finished: List[bool]
    margin: float
    # trace[t][k] = (parent slot, token, score) of slot k after step t; dead: (-1, DEAD, -inf)
    trace: List[List[Tuple[int, int, float]]] = field(default_factory=list)


def step_candidates(slots: Sequence[Optional[Slot]], lps: Dict[int, np.ndarray], norm, banned,
                    keep: int):
    """Every slot's best ``keep`` candidates as (key, slot, token, score, n), unsorted."""
    cands = []
    for k, s in enumerate(slots):
        if s is None:
            continue
        if s.fin:
            cands.append((s.score / norm[s.n], k, CARRIED, s.score, s.n))
            continue
        lp = np.asarray(lps[k], np.float64)
        sc = s.score + lp
        ok = np.ones(lp.shape[0], bool)
        ok[[b for b in banned if 0 <= b < lp.shape[0]]] = False
        ids = np.nonzero(ok)[0]
        order = ids[np.lexsort((ids, -sc[ids]))][:keep]
        for v in order:
            cands.append((float(sc[v]) / norm[s.n + 1], k, int(v), float(sc[v]), s.n + 1))
    return cands


def rank(cands):
    return sorted(cands, key=lambda c: (-c[0], c[1], c[2]))


def beam_search(logp: Callable[[List[List[int]]], Sequence[np.ndarray]], N: int, L: int,
                alpha: float = 0.0, special: Optional[Dict[str, int]] = None,
                alive: bool = True) -> AttResult:
    ids = dict(SPECIAL, **(special or {}))
    banned = {ids["pad"], ids["bos"], ids["blank"]}
    eos = ids["eos"]
    norm = length_norm(L, alpha)
    slots: List[Optional[Slot]] = [Slot([], 0.0, 0, False) if alive else None] + [None] * (N - 1)
    margin = math.inf
    trace = []
    for _ in range(L):
        live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
        out = logp([slots[k].toks for k in live]) if live else []
        ranked = rank(step_candidates(slots, dict(zip(live, out)), norm, banned, N + 1))
        if len(ranked) > N:
            margin = min(margin, ranked[N - 1][0] - ranked[N][0])
        new: List[Optional[Slot]] = []
        row = []
        for key, k, v, sc, n in ranked[:N]:
            s = slots[k]
            if v == CARRIED:
                new.append(Slot(list(s.toks), sc, n, True))
            else:
                new.append(Slot(s.toks + ([] if v == eos else [v]), sc, n, v == eos))
            row.append((k, v, sc))
        while len(new) < N:
            new.append(None)
            row.append((-1, DEAD, NEG_INF))
        slots = new
        trace.append(row)
    alive_slots = [s for s in slots if s is not None]
    keys = [s.score / norm[s.n] for s in alive_slots]
    for a, b in zip(keys, keys[1:]):
        margin = min(margin, a - b)
    return AttResult([s.toks for s in alive_slots], [s.score for s in alive_slots],
                     [s.fin for s in alive_slots], margin, trace)


def table_logp(table: Dict[str, Sequence[float]], default: Sequence[float]):
    """``logp`` from fixed per-prefix tables: key = the prefix's tokens joined by ','."""
    def logp(prefixes):
        return [np.asarray(table.get(",".join(map(str, p)), default), np.float64)
                for p in prefixes]
    return logp


def model_logp(model64, enc: np.ndarray, mask: np.ndarray, bos: int = SPECIAL["bos"]):
    """``logp`` of one utterance from the float64 model, no cache: enc [T', d], mask [T']."""
    import torch

    e = torch.from_numpy(np.asarray(enc, np.float64)[None])
    m = torch.from_numpy(np.asarray(mask)[None])

    def logp(prefixes):
        n = len(prefixes)
        inp = torch.tensor([[bos] + list(p) for p in prefixes], dtype=torch.long)
        with torch.no_grad():
            z = model64.decode_logits(e.repeat(n, 1, 1), m.repeat(n, 1), inp,
                                      torch.zeros(inp.shape, dtype=torch.bool))
        return torch.log_softmax(z[:, -1], dim=-1).numpy()
    return logp


def ancestry(trace, N: int, L: int, row0: int = 0):
    """The ancestry table after the last step from the trace alone: anc[k][j] = row0 + the slot
    that held position j of slot k's prefix (dead slots: their own row)."""
    anc = [[row0 + k] * L for k in range(N)]
    for t, row in enumerate(trace):
        new = []
        for k, (par, _, _) in enumerate(row):
            p = k if par < 0 else par
            new.append(anc[p][:t] + [row0 + p] + [row0 + k] * (L - t - 1))
        anc = new
    return anc


def walk_trace(tp, tt, ts, N: int, eos: int, alive: bool = True):
    """The slots after every step from a trace ([L][N] parent / token / score): a list of L + 1
    lists of N slots (None = dead), entry 0 the state before step 0. Asserts the trace is
    consistent: a carried slot was finished and keeps its score, a token extends a live slot."""
    slots: List[Optional[Slot]] = [Slot([], 0.0, 0, False) if alive else None] + [None] * (N - 1)
    hist = [slots]
    for t in range(len(tp)):
        new: List[Optional[Slot]] = []
        for k in range(N):
            p, v, s = int(tp[t][k]), int(tt[t][k]), float(ts[t][k])
            if v == DEAD:
                assert p == -1 and s == NEG_INF, (t, k, p, s)
                new.append(None)
                continue
            par = slots[p]
            assert par is not None, (t, k, p)
            if v == CARRIED:
                assert par.fin and s == par.score, (t, k)
                new.append(Slot(list(par.toks), s, par.n, True))
            else:
                assert not par.fin and v >= 0, (t, k, v)
                new.append(Slot(par.toks + ([] if v == eos else [v]), s, par.n + 1, v == eos))
        hist.append(new)
        slots = new
    return hist


def check_search(tp, tt, ts, logp64, logp_old, N: int, L: int, alpha: float = 0.0,
                 special: Optional[Dict[str, int]] = None, alive: bool = True):
    """The step-wise rule for one utterance's device trace. For the device's own beams at every
    step the oracle ``logp64`` scores every candidate in float64; ``logp_old`` is the existing
    path on the same prefixes. With e = 4 x the existing path's largest score error over the
    selected candidates: (a) every selected candidate's device score is within e of the oracle's,
    (b) no unselected candidate's oracle key exceeds the smallest selected oracle key by more
    than 2e, (c) the device order is non-increasing in oracle key up to 2e.
    Returns (e, the largest device score error, the slots after the last step)."""
    ids = dict(SPECIAL, **(special or {}))
    banned = sorted({ids["pad"], ids["bos"], ids["blank"]})
    eos = ids["eos"]
    norm = length_norm(L, alpha)
    hist = walk_trace(tp, tt, ts, N, eos, alive)
    # oracle / existing-path score of every slot, keyed by (step, slot)
    o_sc = {(0, 0): 0.0}
    x_sc = {(0, 0): 0.0}
    steps = []
    for t in range(L):
        slots = hist[t]
        live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
        lp64 = dict(zip(live, logp64([slots[k].toks for k in live]))) if live else {}
        lpx = dict(zip(live, logp_old([slots[k].toks for k in live]))) if live else {}
        sel = []          # (oracle key, oracle score, existing score, device score) in slot order
        chosen = {k: [] for k in live}
        for k2, s2 in enumerate(hist[t + 1]):
            if s2 is None:
                continue
            p, v = int(tp[t][k2]), int(tt[t][k2])
            if v == CARRIED:
                o, x = o_sc[(t, p)], x_sc[(t, p)]
            else:
                o = o_sc[(t, p)] + float(lp64[p][v])
                x = x_sc[(t, p)] + float(lpx[p][v])
                assert v not in banned
                chosen[p].append(v)
            o_sc[(t + 1, k2)], x_sc[(t + 1, k2)] = o, x
            sel.append((o / norm[s2.n], o, x, s2.score))
        best_left = NEG_INF   # the best oracle key among the candidates that were not selected
        for k in live:
            sc = o_sc[(t, k)] + np.asarray(lp64[k], np.float64)
            sc[banned] = NEG_INF
            sc[chosen[k]] = NEG_INF
            best_left = max(best_left, float(sc.max()) / norm[slots[k].n + 1])
        carried = {int(tp[t][k2]) for k2 in range(N) if int(tt[t][k2]) == CARRIED}
        for k, s in enumerate(slots):
            if s is not None and s.fin and k not in carried:
                best_left = max(best_left, o_sc[(t, k)] / norm[s.n])
        steps.append((sel, best_left))
    e = 4.0 * max([abs(x - o) for sel, _ in steps for _, o, x, _ in sel] or [0.0])
    worst = 0.0
    for t, (sel, best_left) in enumerate(steps):
        for key, o, _, d in sel:
            worst = max(worst, abs(d - o))
            assert abs(d - o) <= e, (t, d, o, e)                       # (a)
        if sel:
            assert best_left <= min(k for k, *_ in sel) + 2 * e, (t, best_left, e)   # (b)
        for (ka, *_), (kb, *_) in zip(sel, sel[1:]):
            assert kb <= ka + 2 * e, (t, ka, kb, e)                    # (c)
    return e, worst, hist[-1]
