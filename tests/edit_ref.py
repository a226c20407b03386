"""Test helper (not a test): the oracle of the device edit distance, the n-best distances and the
minimum-Bayes-risk pick (``onebit_asr.edit``, csrc/edit.hip). Plain Python and numpy.

``edit_ops(a, b)``: a the reference, b the hypothesis; a cell is (d, sub, ins, del).
D[0][j] = (j, 0, j, 0); D[i][0] = (i, 0, 0, i); a[i-1] == b[j-1] copies D[i-1][j-1]; otherwise
the candidate with the smallest d among diagonal D[i-1][j-1] (a substitution), up D[i-1][j] (a
deletion of a reference token) and left D[i][j-1] (an insertion of a hypothesis token) wins,
ties in that order, and d and the winner's count grow by 1. The result is D[len a][len b].

``edit_distance_np(a, b)``: d alone, one numpy row per reference token (for long inputs).

``mbr(dpair, scores, n, scale)``: over the n live entries, in float64 and ascending index
order, every product and sum rounded on its own: m = max score, w_j = exp(scale (score_j - m))
(0 for score_j = -inf), Z = sum w_j, post_j = w_j / Z, risk_k = sum_j post_j dpair[k][j]; the
smallest risk wins, ties to the smaller k. No live entry, or a largest score of -inf: entry 0,
every risk +inf, every post 0.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np


def edit_ops(a: Sequence, b: Sequence) -> Tuple[int, int, int, int]:
    prev = [(j, 0, j, 0) for j in range(len(b) + 1)]
    for i, x in enumerate(a, 1):
        cur = [(i, 0, 0, i)] + [None] * len(b)
        for j, y in enumerate(b, 1):
            if x == y:
                cur[j] = prev[j - 1]
                continue
            dg, up, lf = prev[j - 1], prev[j], cur[j - 1]
            best, which = dg, 1
            if up[0] < best[0]:
                best, which = up, 3
            if lf[0] < best[0]:
                best, which = lf, 2
            c = list(best)
            c[0] += 1
            c[which] += 1
            cur[j] = tuple(c)
        prev = cur
    return prev[len(b)]


def edit_distance_np(a: Sequence[int], b: Sequence[int]) -> int:
    """d = D[len a][len b]. A row is min(diagonal or substitution, deletion) followed by the
    insertion chain cur[j] = min(cur[j], cur[j-1] + 1), which is a running minimum of
    cur[j] - j."""
    b = np.asarray(b, dtype=np.int64)
    idx = np.arange(len(b) + 1, dtype=np.int64)
    prev = idx.copy()
    for i, x in enumerate(a, 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (b != x), prev[1:] + 1)
        prev = np.minimum.accumulate(cur - idx) + idx
    return int(prev[len(b)])


def pairwise(entries: Sequence[Sequence[int]], n: int, N: int) -> List[List[int]]:
    """dpair [N][N] of the first n entries: symmetric, 0 on the live diagonal, -1 elsewhere."""
    d = [[-1] * N for _ in range(N)]
    for j in range(n):
        d[j][j] = 0
        for k in range(j + 1, n):
            d[j][k] = d[k][j] = edit_ops(entries[j], entries[k])[0]
    return d


def mbr(dpair: Sequence[Sequence[int]], scores: Sequence[float], n: int, scale: float
        ) -> Tuple[int, List[float], List[float]]:
    """(best_k, risk [N], post [N]) by the rule above."""
    N = len(scores)
    risk, post = [math.inf] * N, [0.0] * N
    m = -math.inf
    for j in range(n):
        if scores[j] > m:
            m = scores[j]
    if not m > -math.inf:
        return 0, risk, post
    w = [math.exp(scale * (scores[j] - m)) if scores[j] > -math.inf else 0.0 for j in range(n)]
    z = 0.0
    for j in range(n):
        z += w[j]
    for j in range(n):
        post[j] = w[j] / z
    for k in range(n):
        r = 0.0
        for j in range(n):
            r += post[j] * float(dpair[k][j])
        risk[k] = r
    best = 0
    for k in range(1, n):
        if risk[k] < risk[best]:
            best = k
    return best, risk, post
