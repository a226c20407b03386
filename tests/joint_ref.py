"""Test helper (not a test): the float64 oracle of the joint CTC/attention beam search
(``onebit_asr.attdec.joint_beam_search``, csrc/ctcprefix.hip).

CTC prefix state of a prefix g over the T valid frames, x [T, V] the float64 log-softmax of the
CTC logits: gn[t] / gb[t] = log P(frames 0..t emit exactly g and end in a non-blank / a blank).

* ``root`` / ``extend`` / ``eos_score``: the recursion (Watanabe et al. 2017), plain Python
  floats. ``extend`` returns (hn, hb, psi), psi = log P(the transcript starts with g . c).
* ``brute_force``: the same two quantities by enumerating every alignment.
* ``joint_search``: the search, a function of ``logp`` (as ``attdec_ref.beam_search``) and x.
  Every live slot offers its K best attention candidates (float64 order, ties to the smaller
  id); candidate (r, c) has A' = A_r + lp_r[c], C' = psi(g_r . c) -- for eos
  lse(gn[T-1], gb[T-1]) --, is dropped when w > 0 and C' = -inf, and scores
  S' = (1 - w) * A' + w * C' (w == 0: S' = A', nothing dropped). Key S / norm[n], the N largest
  survive, ties to the smaller slot, then the smaller token.
* ``check_joint_search``: the step-wise rule for a device trace (see its docstring).
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from attdec_ref import CARRIED, DEAD, NEG_INF, SPECIAL, length_norm, rank, walk_trace


def lse(a: float, b: float) -> float:
    if a == NEG_INF:
        return b
    if b == NEG_INF:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def log_softmax64(z: np.ndarray) -> np.ndarray:
    """x[t][v] = (double)z[t][v] - lse64(z[t]) of fp32 logits [T, V]."""
    z = np.asarray(z, np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))


def root(x: np.ndarray, blank: int) -> Tuple[List[float], List[float]]:
    T = x.shape[0]
    gb, acc = [], 0.0
    for t in range(T):
        acc = acc + float(x[t][blank])
        gb.append(acc)
    return [NEG_INF] * T, gb


def extend(x: np.ndarray, blank: int, g: Sequence[int], gn: Sequence[float],
           gb: Sequence[float], c: int):
    """(hn, hb, psi) of h = g . c from the state of g; c is neither blank nor eos."""
    T = x.shape[0]
    hn = [float(x[0][c]) if len(g) == 0 else NEG_INF]
    hb = [NEG_INF]
    psi = hn[0]
    same = len(g) > 0 and g[-1] == c
    for t in range(1, T):
        phi = gb[t - 1] if same else lse(gn[t - 1], gb[t - 1])
        xc = float(x[t][c])
        hn.append(lse(hn[t - 1], phi) + xc)
        hb.append(lse(hn[t - 1], hb[t - 1]) + float(x[t][blank]))
        psi = lse(psi, phi + xc)
    return hn, hb, psi


def eos_score(gn: Sequence[float], gb: Sequence[float]) -> float:
    return lse(gn[-1], gb[-1])


def prefix_state(x: np.ndarray, blank: int, g: Sequence[int]):
    """(gn, gb, psi) of a whole prefix from the root."""
    gn, gb = root(x, blank)
    psi = 0.0
    for i, c in enumerate(g):
        gn, gb, psi = extend(x, blank, g[:i], gn, gb, c)
    return gn, gb, psi


def brute_force(x: np.ndarray, blank: int, g: Sequence[int]) -> Tuple[float, float]:
    """(log P(transcript starts with g), log P(transcript == g)) over all V ** T alignments."""
    T, V = x.shape
    g = list(g)
    starts, full = [], []
    for path in itertools.product(range(V), repeat=T):
        out, prev = [], None
        for s in path:
            if s != prev and s != blank:
                out.append(s)
            prev = s
        lp = float(sum(x[t][s] for t, s in enumerate(path)))
        if out[:len(g)] == g:
            starts.append(lp)
        if out == g:
            full.append(lp)

    def total(v):
        if not v:
            return NEG_INF
        m = max(v)
        return m + math.log(math.fsum(math.exp(a - m) for a in v))
    return total(starts), total(full)


# ------------------------------------------------------------------------------------------
# the search
# ------------------------------------------------------------------------------------------
@dataclass
class JSlot:
    toks: List[int]
    A: float
    C: float
    S: float
    n: int
    fin: bool
    gn: Optional[List[float]] = None
    gb: Optional[List[float]] = None


@dataclass
class JointResult:
    hyps: List[List[int]]
    scores: List[float]              # S
    att: List[float]
    ctc: List[float]
    finished: List[bool]
    margin: float                    # the smallest key gap at a decision, final ranking included
    dropped: int                     # candidates dropped as CTC-impossible
    trace: List[List[Tuple[int, int, float]]] = field(default_factory=list)
    slots: List[Optional[JSlot]] = field(default_factory=list)
    history: List[List[Optional[JSlot]]] = field(default_factory=list)   # [L + 1] slot lists


def combine(w: float, a: float, c: float) -> float:
    return a if w == 0 else (1.0 - w) * a + w * c


def top_candidates(lp: np.ndarray, banned, K: int) -> np.ndarray:
    """The K best ids outside ``banned``: value descending, ties to the smaller id."""
    ids = np.array([v for v in range(lp.shape[0]) if v not in banned])
    return ids[np.lexsort((ids, -lp[ids]))][:K]


def slot_candidates(s: JSlot, k: int, lp: np.ndarray, x: np.ndarray, ids, banned, K: int,
                    w: float, norm, cscore=None):
    """-> (kept candidates as (key, slot, token, S, A, C, n, gn, gb), dropped count).
    ``cscore(prefix, token)``: a table in place of the recursion (bookkeeping tests)."""
    out, dropped = [], 0
    for v in top_candidates(lp, banned, K):
        v = int(v)
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
        sc = combine(w, a, c)
        out.append((sc / norm[s.n + 1], k, v, sc, a, c, s.n + 1, gn, gb))
    return out, dropped


def joint_search(logp: Callable[[List[List[int]]], Sequence[np.ndarray]], x: np.ndarray, N: int,
                 K: int, L: int, w: float, alpha: float = 0.0,
                 special: Optional[Dict[str, int]] = None, alive: bool = True,
                 cscore=None) -> JointResult:
    ids = dict(SPECIAL, **(special or {}))
    banned = {ids["pad"], ids["bos"], ids["blank"]}
    norm = length_norm(L, alpha)
    first = None
    if alive:
        gn, gb = root(x, ids["blank"]) if w > 0 and cscore is None else (None, None)
        first = JSlot([], 0.0, 0.0, 0.0, 0, False, gn, gb)
    slots: List[Optional[JSlot]] = [first] + [None] * (N - 1)
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
                cands.append((s.S / norm[s.n], k, CARRIED, s.S, s.A, s.C, s.n, None, None))
                continue
            got, d = slot_candidates(s, k, np.asarray(lps[k], np.float64), x, ids, banned, K, w,
                                     norm, cscore)
            cands += got
            dropped += d
        ranked = rank(cands)
        if len(ranked) > N:
            margin = min(margin, ranked[N - 1][0] - ranked[N][0])
        new: List[Optional[JSlot]] = []
        row = []
        for key, k, v, sc, a, c, n, gn, gb in ranked[:N]:
            s = slots[k]
            if v == CARRIED:
                new.append(JSlot(list(s.toks), a, c, sc, n, True))
            elif v == ids["eos"]:
                new.append(JSlot(list(s.toks), a, c, sc, n, True))
            else:
                new.append(JSlot(s.toks + [v], a, c, sc, n, False, gn, gb))
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
    return JointResult([s.toks for s in alive_slots], [s.S for s in alive_slots],
                       [s.A for s in alive_slots], [s.C for s in alive_slots],
                       [s.fin for s in alive_slots], margin, dropped, trace, slots, history)


def check_joint_search(tp, tt, ts, logp64, logp_old, x: np.ndarray, N: int, K: int, L: int,
                       w: float, alpha: float = 0.0, special: Optional[Dict[str, int]] = None,
                       alive: bool = True):
    """The step-wise rule for one utterance's device trace (w > 0). For the device's own beams at
    every step the oracle scores every candidate: A from ``logp64``, C from the recursion on x;
    ``logp_old`` is the existing attention path on the same prefixes. With e = 4 x the existing
    path's largest error of A over the selected candidates + 1e-9 * max(1, T):
    (a) every selected candidate's device S is within e of the oracle's (so none is one the
        oracle drops);
    (b) no unselected, undropped candidate inside the oracle's attention top-K has an oracle key
        above the smallest selected oracle key + 2e;
    (c) the device order is non-increasing in oracle key up to 2e;
    (p) every selected token's oracle attention log-probability is at least the row's K-th
        largest - 2e.
    Returns (e, the largest device S error, per-slot (A, C) of the oracle after the last step,
    the slots after the last step, the number of top-K candidates the oracle drops)."""
    ids = dict(SPECIAL, **(special or {}))
    banned = sorted({ids["pad"], ids["bos"], ids["blank"]})
    eos, blank = ids["eos"], ids["blank"]
    T = x.shape[0]
    norm = length_norm(L, alpha)
    hist = walk_trace(tp, tt, ts, N, eos, alive)
    o_a, x_a, o_c = {(0, 0): 0.0}, {(0, 0): 0.0}, {(0, 0): 0.0}
    state = {(0, 0): root(x, blank)}
    steps, dropped = [], 0
    for t in range(L):
        slots = hist[t]
        live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
        lp64 = dict(zip(live, logp64([slots[k].toks for k in live]))) if live else {}
        lpx = dict(zip(live, logp_old([slots[k].toks for k in live]))) if live else {}
        # the oracle's view of every top-K candidate of every live row
        cand = {}
        kth = {}
        for k in live:
            lp = np.asarray(lp64[k], np.float64)
            top = top_candidates(lp, banned, K)
            kth[k] = float(lp[top[-1]]) if len(top) == K else NEG_INF
            gn, gb = state[(t, k)]
            for v in map(int, top):
                if v == eos:
                    cand[(k, v)] = (eos_score(gn, gb), None)
                else:
                    hn, hb, psi = extend(x, blank, slots[k].toks, gn, gb, v)
                    cand[(k, v)] = (psi, (hn, hb))
        sel, chosen = [], set()
        for k2, s2 in enumerate(hist[t + 1]):
            if s2 is None:
                continue
            p, v = int(tp[t][k2]), int(tt[t][k2])
            if v == CARRIED:
                a, xa, c = o_a[(t, p)], x_a[(t, p)], o_c[(t, p)]
            else:
                assert v not in banned
                lp = float(lp64[p][v])
                a = o_a[(t, p)] + lp
                xa = x_a[(t, p)] + float(lpx[p][v])
                if (p, v) in cand:
                    c, st = cand[(p, v)]
                elif v == eos:
                    c, st = eos_score(*state[(t, p)]), None
                else:
                    hn, hb, c = extend(x, blank, slots[p].toks, *state[(t, p)], v)
                    st = (hn, hb)
                if st is not None:
                    state[(t + 1, k2)] = st
                chosen.add((p, v))
                sel.append(("p", lp, kth[p]))
            o_a[(t + 1, k2)], x_a[(t + 1, k2)], o_c[(t + 1, k2)] = a, xa, c
            so = combine(w, a, c)
            sel.append((so / norm[s2.n], so, a, xa, s2.score))
        best_left = NEG_INF
        for (k, v), (c, _) in cand.items():
            if (k, v) in chosen:
                continue
            if c == NEG_INF:
                dropped += 1
                continue
            so = combine(w, o_a[(t, k)] + float(lp64[k][v]), c)
            best_left = max(best_left, so / norm[slots[k].n + 1])
        carried = {int(tp[t][k2]) for k2 in range(N) if int(tt[t][k2]) == CARRIED}
        for k, s in enumerate(slots):
            if s is not None and s.fin and k not in carried:
                best_left = max(best_left, combine(w, o_a[(t, k)], o_c[(t, k)]) / norm[s.n])
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
    final = [None if s is None else (o_a[(L, k)], o_c[(L, k)]) for k, s in enumerate(last)]
    return e, worst, final, last, dropped


def hash_logp(seed: int, V: int, eos: int):
    """A deterministic per-prefix table of binary fractions (multiples of 1/64 in [-8, 0]): every
    float64 sum is exact and ties are frequent (as test_attdec_gpu's table)."""
    import zlib

    def logp(prefixes):
        out = []
        for p in prefixes:
            rng = np.random.default_rng(zlib.crc32(repr((seed, tuple(p))).encode()))
            lp = -rng.integers(0, 513, size=V).astype(np.float64) / 64.0
            if rng.random() < 0.3:
                lp[eos] = -rng.integers(0, 16) / 64.0
            out.append(lp)
        return out
    return logp
