"""Test helper (not a test): the oracle of the n-gram LM shallow fusion (onebit_asr/ngram.py,
csrc/ngram.hip, the fused step of csrc/attdec.hip).

* ``RefLM``: the scoring rule over a Python dict. ``entries`` maps an id tuple to (logp, backoff);
  values are rounded to float32 once, the sum is Python float (float64) in the rule's order:

      prefix = [bos] + tokens;  h = its last min(order - 1, len(prefix)) ids
      acc = 0
      for m = len(h) .. 0:
          if (h[-m:], w) is an entry:        return acc + logp
          if m >= 1 and h[-m:] is an entry:  acc += backoff
      return acc + unk_logp

  ``score_detail`` also names the outcome: ``hit1``..``hit4`` (the order of the entry that ended
  the sum), ``unk``; plus the flags ``backoff_full`` (ended below the longest context and every
  context on the way was an entry), ``ctx_missing`` (a context on the way was no entry, so no
  back-off was added for it), ``short`` (the prefix is shorter than order - 1).
* ``fused_search``: ``joint_ref.joint_search`` with the LM term: a candidate also has
  Lm' = Lm_r + score(g_r, c) and S' = combine(w, A', C') + lm_weight * Lm'.
* ``check_fused_search``: ``joint_ref.check_joint_search``'s step-wise rule with the LM term, which
  is exact and adds no error of its own.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from attdec_ref import CARRIED, DEAD, NEG_INF, SPECIAL, length_norm, rank, walk_trace
from joint_ref import combine, eos_score, extend, root, top_candidates

BOS, EOS = 1, 2


class RefLM:
    def __init__(self, entries: Dict[Tuple[int, ...], Tuple[float, float]], order: int,
                 unk_logp: Optional[float] = None):
        self.order = order
        self.entries = {tuple(int(i) for i in g): (float(np.float32(lp)), float(np.float32(bo)))
                        for g, (lp, bo) in entries.items()}
        self.unk = float(np.float32(math.log(1e-10) if unk_logp is None else unk_logp))

    def context(self, tokens: Sequence[int]) -> List[int]:
        prefix = [BOS] + [int(t) for t in tokens]
        k = min(self.order - 1, len(prefix))
        return prefix[len(prefix) - k:]

    def score_detail(self, tokens: Sequence[int], w: int):
        """-> (log P(w | [bos] + tokens), the set of outcome labels)."""
        if w < 0:
            return NEG_INF, {"absent"}
        h = self.context(tokens)
        tags = set()
        if len(h) < self.order - 1:
            tags.add("short")
        acc, added, missing = 0.0, 0, 0
        for m in range(len(h), -1, -1):
            ctx = tuple(h[len(h) - m:])
            e = self.entries.get(ctx + (int(w),))
            if e is not None:
                tags.add(f"hit{m + 1}")
                if m < len(h) and missing == 0:
                    tags.add("backoff_full")
                if missing:
                    tags.add("ctx_missing")
                return acc + e[0], tags
            if m >= 1:
                c = self.entries.get(ctx)
                if c is not None:
                    acc += c[1]
                    added += 1
                else:
                    missing += 1
        tags.add("unk")
        if missing:
            tags.add("ctx_missing")
        return acc + self.unk, tags

    def score(self, tokens: Sequence[int], w: int) -> float:
        return self.score_detail(tokens, w)[0]

    def seq_scores(self, tokens: Sequence[int]) -> List[float]:
        toks = [int(t) for t in tokens]
        return [self.score(toks[:j], w) for j, w in enumerate(toks + [EOS])]

    def seq_logprob(self, tokens: Sequence[int]) -> float:
        total = 0.0
        for s in self.seq_scores(tokens):
            total += s
        return total


def random_lm(seed: int, order: int, V: int, n_entries: int, reserved=(0, 1, 3)):
    """A random back-off table: (entries dict, ids [E, 4], n [E], vals float32 [E, 2]). Every
    longer n-gram's context is usually an entry too (as in a real model), a few are left out;
    logp / backoff are arbitrary float32 values (not binary fractions: the sums round)."""
    rng = np.random.default_rng(seed)
    words = np.array([v for v in range(V) if v not in reserved and v != BOS], np.int64)
    firsts = np.concatenate([words[words != EOS], [BOS]])      # a context may start with bos
    entries: Dict[Tuple[int, ...], Tuple[float, float]] = {}
    # (a tenth of the words get no unigram: unknown tokens)
    n_uni = min(max(1, len(words) * 9 // 10), max(1, n_entries // 4) if order > 1 else n_entries)
    for w in rng.choice(words, size=n_uni, replace=False):
        entries[(int(w),)] = (float(np.float32(-rng.uniform(0.5, 9.0))),
                              float(np.float32(-rng.uniform(0.0, 2.0))))
    if order > 1:
        entries[(BOS,)] = (float(np.float32(-99.0)), float(np.float32(-rng.uniform(0.0, 2.0))))
    per = (n_entries - len(entries)) // max(order - 1, 1)
    prev = list(entries)
    for n in range(2, order + 1):
        grams = set()
        cand_prev = [g for g in prev if g[-1] != EOS]
        pick = rng.integers(0, len(cand_prev), size=2 * per)
        nxt = rng.choice(words, size=2 * per)
        for i, w in zip(pick, nxt):
            if len(grams) >= per:
                break
            g = cand_prev[int(i)]
            if rng.random() < 0.1:                              # a context that is no entry
                g = (int(rng.choice(firsts)),) + g[1:] if len(g) > 1 else (int(rng.choice(firsts)),)
            grams.add(g + (int(w),))
        for g in grams:
            entries[g] = (float(np.float32(-rng.uniform(0.1, 8.0))),
                          float(np.float32(-rng.uniform(0.0, 2.0))) if n < order else 0.0)
        prev = list(grams)
    ids = np.zeros((len(entries), 4), np.int64)
    n_arr = np.zeros(len(entries), np.int64)
    vals = np.zeros((len(entries), 2), np.float32)
    for i, (g, (lp, bo)) in enumerate(entries.items()):
        ids[i, :len(g)] = g
        n_arr[i] = len(g)
        vals[i] = (lp, bo)
    return entries, ids, n_arr, vals


@functools.lru_cache(maxsize=None)
def big_lm(seed: int = 4242, order: int = 4, V: int = 5004, n_entries: int = 200_000):
    """The shared random table of the bit-for-bit tests: (RefLM, ids, n, vals)."""
    entries, ids, n, vals = random_lm(seed, order, V, n_entries)
    return RefLM(entries, order), ids, n, vals


def draw_queries(ref: RefLM, V: int, count: int, seed: int):
    """(prefix tokens, candidate) pairs that exercise every outcome: contexts and candidates taken
    from the table's own n-grams (hits at every order, full back-off), random contexts (contexts
    that are no entries), arbitrary candidates (unknown tokens among them), prefixes of 0..5
    tokens (shorter than the order among them), a few absent candidates (-1)."""
    rng = np.random.default_rng(seed)
    grams = list(ref.entries)
    out = []
    for i in range(count):
        g = grams[int(rng.integers(len(grams)))]
        kind = i % 6
        if kind == 0:                                   # the n-gram itself
            toks, w = list(g[:-1]), g[-1]
        elif kind == 1:                                 # its context, another known last word
            toks, w = list(g[:-1]), grams[int(rng.integers(len(grams)))][-1]
        elif kind == 2:                                 # a longer history ahead of it
            toks, w = [int(rng.integers(4, V))] * int(rng.integers(0, 3)) + list(g[:-1]), g[-1]
        elif kind == 3:                                 # a random context
            toks = [int(v) for v in rng.integers(4, V, size=int(rng.integers(0, 6)))]
            w = g[-1]
        elif kind == 4:                                 # any candidate
            toks, w = list(g[:-1]), int(rng.integers(0, V))
        else:
            toks, w = list(g), (-1 if i % 30 == 5 else g[0])
        if toks and toks[0] == BOS:
            toks = toks[1:]                             # (the prefix gets its bos itself)
        out.append(([t for t in toks if t != BOS], int(w)))
    return out


# ------------------------------------------------------------------------------------------
# the fused search
# ------------------------------------------------------------------------------------------
@dataclass
class FSlot:
    toks: List[int]
    A: float
    C: float
    Lm: float
    S: float
    n: int
    fin: bool
    gn: Optional[List[float]] = None
    gb: Optional[List[float]] = None

    @property
    def score(self):
        return self.S


@dataclass
class FusedResult:
    hyps: List[List[int]]
    scores: List[float]
    att: List[float]
    ctc: List[float]
    lm: List[float]
    finished: List[bool]
    margin: float
    dropped: int
    trace: List[List[Tuple[int, int, float]]] = field(default_factory=list)
    history: List[List[Optional[FSlot]]] = field(default_factory=list)


def fuse(w: float, lw: float, a: float, c: float, lm: float) -> float:
    """((1 - w) * A + w * C) + lw * Lm, every operation rounded (w == 0: A + lw * Lm)."""
    return combine(w, a, c) + lw * lm


def fused_search(logp: Callable[[List[List[int]]], Sequence[np.ndarray]], x: np.ndarray,
                 lm: RefLM, N: int, K: int, L: int, w: float, lw: float, alpha: float = 0.0,
                 special: Optional[Dict[str, int]] = None, alive: bool = True,
                 cscore=None) -> FusedResult:
    ids = dict(SPECIAL, **(special or {}))
    banned = {ids["pad"], ids["bos"], ids["blank"]}
    norm = length_norm(L, alpha)
    first = None
    if alive:
        gn, gb = root(x, ids["blank"]) if w > 0 and cscore is None else (None, None)
        first = FSlot([], 0.0, 0.0, 0.0, 0.0, 0, False, gn, gb)
    slots: List[Optional[FSlot]] = [first] + [None] * (N - 1)
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
                cands.append((s.S / norm[s.n], k, CARRIED, s.S, s.A, s.C, s.Lm, s.n, None, None))
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
                l_ = s.Lm + lm.score(s.toks, v)
                sc = fuse(w, lw, a, c, l_)
                cands.append((sc / norm[s.n + 1], k, v, sc, a, c, l_, s.n + 1, gn, gb))
        ranked = rank(cands)
        if len(ranked) > N:
            margin = min(margin, ranked[N - 1][0] - ranked[N][0])
        new: List[Optional[FSlot]] = []
        row = []
        for key, k, v, sc, a, c, l_, n, gn, gb in ranked[:N]:
            s = slots[k]
            if v == CARRIED or v == ids["eos"]:
                new.append(FSlot(list(s.toks), a, c, l_, sc, n, True))
            else:
                new.append(FSlot(s.toks + [v], a, c, l_, sc, n, False, gn, gb))
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
    return FusedResult([s.toks for s in alive_slots], [s.S for s in alive_slots],
                       [s.A for s in alive_slots], [s.C for s in alive_slots],
                       [s.Lm for s in alive_slots], [s.fin for s in alive_slots], margin, dropped,
                       trace, history)


def check_fused_search(tp, tt, ts, logp64, logp_old, x: np.ndarray, lm: RefLM, N: int, K: int,
                       L: int, w: float, lw: float, alpha: float = 0.0,
                       special: Optional[Dict[str, int]] = None, alive: bool = True):
    """``joint_ref.check_joint_search``'s rule (a), (b), (c), (p) for a device trace of the fused
    search, S = fuse(w, lw, A, C, Lm); w == 0 means no CTC term (C = 0, nothing dropped). The LM
    term is exact, so e is as there: 4 x the existing attention path's largest error of A over the
    selected candidates + 1e-9 * max(1, T).
    Returns (e, the largest device S error, per-slot (A, C, Lm) of the oracle after the last step,
    the slots after the last step, the number of top-K candidates the oracle drops)."""
    ids = dict(SPECIAL, **(special or {}))
    banned = sorted({ids["pad"], ids["bos"], ids["blank"]})
    eos, blank = ids["eos"], ids["blank"]
    T = x.shape[0]
    norm = length_norm(L, alpha)
    hist = walk_trace(tp, tt, ts, N, eos, alive)
    o_a, x_a, o_c, o_l = {(0, 0): 0.0}, {(0, 0): 0.0}, {(0, 0): 0.0}, {(0, 0): 0.0}
    state = {(0, 0): root(x, blank) if w > 0 else (None, None)}
    steps, dropped = [], 0

    def ctc_of(toks, st, v):
        if w == 0:
            return 0.0, (None, None)
        if v == eos:
            return eos_score(*st), None
        hn, hb, psi = extend(x, blank, toks, st[0], st[1], v)
        return psi, (hn, hb)

    for t in range(L):
        slots = hist[t]
        live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
        lp64 = dict(zip(live, logp64([slots[k].toks for k in live]))) if live else {}
        lpx = dict(zip(live, logp_old([slots[k].toks for k in live]))) if live else {}
        cand, kth = {}, {}
        for k in live:
            lp = np.asarray(lp64[k], np.float64)
            top = top_candidates(lp, banned, K)
            kth[k] = float(lp[top[-1]]) if len(top) == K else NEG_INF
            for v in map(int, top):
                cand[(k, v)] = ctc_of(slots[k].toks, state[(t, k)], v)
        sel, chosen = [], set()
        for k2, s2 in enumerate(hist[t + 1]):
            if s2 is None:
                continue
            p, v = int(tp[t][k2]), int(tt[t][k2])
            if v == CARRIED:
                a, xa, c, l_ = o_a[(t, p)], x_a[(t, p)], o_c[(t, p)], o_l[(t, p)]
            else:
                assert v not in banned
                lp = float(lp64[p][v])
                a = o_a[(t, p)] + lp
                xa = x_a[(t, p)] + float(lpx[p][v])
                c, st = cand[(p, v)] if (p, v) in cand else ctc_of(slots[p].toks, state[(t, p)], v)
                if st is not None:
                    state[(t + 1, k2)] = st
                l_ = o_l[(t, p)] + lm.score(slots[p].toks, v)
                chosen.add((p, v))
                sel.append(("p", lp, kth[p]))
            o_a[(t + 1, k2)], x_a[(t + 1, k2)] = a, xa
            o_c[(t + 1, k2)], o_l[(t + 1, k2)] = c, l_
            so = fuse(w, lw, a, c, l_)
            sel.append((so / norm[s2.n], so, a, xa, s2.score))
        best_left = NEG_INF
        for (k, v), (c, _) in cand.items():
            if (k, v) in chosen:
                continue
            if w > 0 and c == NEG_INF:
                dropped += 1
                continue
            so = fuse(w, lw, o_a[(t, k)] + float(lp64[k][v]), c,
                      o_l[(t, k)] + lm.score(slots[k].toks, v))
            best_left = max(best_left, so / norm[slots[k].n + 1])
        carried = {int(tp[t][k2]) for k2 in range(N) if int(tt[t][k2]) == CARRIED}
        for k, s in enumerate(slots):
            if s is not None and s.fin and k not in carried:
                best_left = max(best_left, fuse(w, lw, o_a[(t, k)], o_c[(t, k)], o_l[(t, k)])
                                / norm[s.n])
        steps.append((sel, best_left))
    picked = [r for sel, _ in steps for r in sel if r[0] != "p"]
    e = 4.0 * max([abs(xa - a) for _, _, a, xa, _ in picked] or [0.0]) + 1e-9 * max(1, T)
    worst = 0.0
    for t, (sel, best_left) in enumerate(steps):
        rows = [r for r in sel if r[0] != "p"]
        for _, lp, kth_lp in (r for r in sel if r[0] == "p"):
            assert lp >= kth_lp - 2 * e, (t, lp, kth_lp, e)                  # (p)
        for key, so, _, _, d in rows:
            assert so != NEG_INF and d != NEG_INF, (t, so, d)
            worst = max(worst, abs(d - so))
            assert abs(d - so) <= e, (t, d, so, e)                           # (a)
        if rows:
            assert best_left <= min(r[0] for r in rows) + 2 * e, (t, best_left, e)   # (b)
        for ra, rb in zip(rows, rows[1:]):
            assert rb[0] <= ra[0] + 2 * e, (t, ra[0], rb[0], e)              # (c)
    last = hist[-1]
    final = [None if s is None else (o_a[(L, k)], o_c[(L, k)], o_l[(L, k)])
             for k, s in enumerate(last)]
    return e, worst, final, last, dropped
