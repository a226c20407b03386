"""Edit distance on the device (csrc/edit.hip): batched Levenshtein distance over padded int32
sequences, with the substitution / insertion / deletion counts, and what an eval path builds on it.

* ``edit_distance``: distance (and counts) of P (reference, hypothesis) pairs (``ob_edit_distance``);
* ``nbest_edit_distance``: every n-best entry against its utterance's reference, and the pairwise
  distances among the entries, in one launch (``ob_nbest_edit_distance``);
* ``nbest_oracle``: the entry closest to the reference (the oracle error rate of a beam);
* ``mbr_select``: the minimum-Bayes-risk entry of an n-best under the posterior its totals define
  (``ob_mbr_select``).

The definition of a cell, the tie order and the limits are in include/onebit_hip.h. Nothing here
synchronises with the host; the workspaces come from the caching allocator; all of it can be
captured in a HIP graph. ``metrics.token_error_counts`` / ``compute_wer_device`` sum the counts.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple, Union

import torch

from . import _lib

__all__ = ["edit_distance", "nbest_edit_distance", "nbest_oracle", "mbr_select"]

MAX_LEN = 4096     # ob_edit_distance's limits (include/onebit_hip.h)
MAX_NBEST = 32


def _i32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _workspace(need: int, dev) -> torch.Tensor:
    return torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)


def edit_distance(a: torch.Tensor, a_len: torch.Tensor, b: torch.Tensor, b_len: torch.Tensor,
                  ops: bool = False) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """a [P, La] the references and b [P, Lb] the hypotheses (device, int32 or int64, padded with
    anything), a_len / b_len [P] -> dist int32 [P], the Levenshtein distance of every pair; with
    ``ops=True`` (dist, ops int32 [P, 3] = substitutions, insertions, deletions). A length above
    the width is clamped to it; a pair with a negative length is absent: dist and ops -1.
    La, Lb <= 4096."""
    if not a.is_cuda:
        raise RuntimeError("edit_distance runs on the HIP library (no CPU fallback)")
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError(f"edit_distance: a {tuple(a.shape)} / b {tuple(b.shape)} are not "
                         "[P, La] / [P, Lb]")
    p, la = a.shape
    lb = b.shape[1]
    if b.shape[0] != p or a_len.shape != (p,) or b_len.shape != (p,):
        raise ValueError(f"edit_distance: b {tuple(b.shape)}, a_len {tuple(a_len.shape)}, b_len "
                         f"{tuple(b_len.shape)} do not match {p} pairs")
    lib = _lib.load()
    if not lib.ob_edit_supported(la, lb):
        raise ValueError(f"edit_distance: La={la}, Lb={lb} is not supported (both <= {MAX_LEN})")
    dev = a.device
    a, al, b, bl = _i32(a, dev), _i32(a_len, dev), _i32(b, dev), _i32(b_len, dev)
    dist = torch.empty((p,), dtype=torch.int32, device=dev)
    op = torch.empty((p, 3), dtype=torch.int32, device=dev) if ops else None
    need = lib.ob_edit_distance_workspace(p, la, lb)
    if need == 0:
        raise ValueError(f"edit_distance: shape P={p} La={la} Lb={lb} is not supported")
    ws = _workspace(need, dev)
    _lib.check(lib.ob_edit_distance(a.data_ptr(), al.data_ptr(), b.data_ptr(), bl.data_ptr(), p,
                                    la, lb, ws.data_ptr(), ws.numel() * 8, dist.data_ptr(),
                                    _lib.ptr(op), _lib.stream_of(a)), "ob_edit_distance")
    return (dist, op) if ops else dist


def _nbest_args(fn: str, hyp, hyp_len, n_hyp):
    if not hyp.is_cuda:
        raise RuntimeError(f"{fn} runs on the HIP library (no CPU fallback)")
    if hyp.dim() != 3:
        raise ValueError(f"{fn}: hyp {tuple(hyp.shape)} is not [B, N, T]")
    b, n, t = hyp.shape
    if hyp_len.shape != (b, n) or n_hyp.shape != (b,):
        raise ValueError(f"{fn}: hyp_len {tuple(hyp_len.shape)} / n_hyp {tuple(n_hyp.shape)} do "
                         f"not match hyp {tuple(hyp.shape)}")
    if not 1 <= n <= MAX_NBEST or t > MAX_LEN:
        raise ValueError(f"{fn}: N={n}, T={t} is not supported (1 <= N <= {MAX_NBEST}, "
                         f"T <= {MAX_LEN})")
    dev = hyp.device
    return _i32(hyp, dev), _i32(hyp_len, dev), _i32(n_hyp, dev)


def nbest_edit_distance(hyp: torch.Tensor, hyp_len: torch.Tensor, n_hyp: torch.Tensor,
                        ref: Optional[torch.Tensor] = None,
                        ref_len: Optional[torch.Tensor] = None, pairwise: bool = False
                        ) -> Dict[str, torch.Tensor]:
    """hyp [B, N, T] / hyp_len [B, N] / n_hyp [B], an n-best in the decoders' layout. With
    ``ref`` [B, S] / ``ref_len`` [B]: ``dref`` int32 [B, N], the distance of every live entry to its
    utterance's reference, and ``ops`` int32 [B, N, 3] (substitutions, insertions, deletions), -1
    for absent entries k >= n_hyp[b]. With ``pairwise=True``: ``dpair`` int32 [B, N, N], the
    distances among the live entries (symmetric, 0 on their diagonal), -1 in the rows and columns
    of absent entries. One launch for all of it. N <= 32, T, S <= 4096."""
    fn = "nbest_edit_distance"
    hyp, hyp_len, n_hyp = _nbest_args(fn, hyp, hyp_len, n_hyp)
    b, n, t = hyp.shape
    dev = hyp.device
    if (ref is None) != (ref_len is None):
        raise ValueError(f"{fn}: ref and ref_len go together")
    if ref is None and not pairwise:
        raise ValueError(f"{fn}: nothing to compute (no ref and pairwise=False)")
    s = 0
    out: Dict[str, torch.Tensor] = {}
    if ref is not None:
        if ref.dim() != 2 or ref.shape[0] != b or ref_len.shape != (b,):
            raise ValueError(f"{fn}: ref {tuple(ref.shape)} / ref_len {tuple(ref_len.shape)} do "
                             f"not match a batch of {b}")
        s = ref.shape[1]
        ref, ref_len = _i32(ref, dev), _i32(ref_len, dev)
        out["dref"] = torch.empty((b, n), dtype=torch.int32, device=dev)
        out["ops"] = torch.empty((b, n, 3), dtype=torch.int32, device=dev)
    if pairwise:
        out["dpair"] = torch.empty((b, n, n), dtype=torch.int32, device=dev)
    lib = _lib.load()
    need = lib.ob_nbest_edit_distance_workspace(b, n, t, s)
    if need == 0:
        raise ValueError(f"{fn}: shape B={b} N={n} T={t} S={s} is not supported (S <= {MAX_LEN})")
    ws = _workspace(need, dev)
    _lib.check(lib.ob_nbest_edit_distance(
        hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(), _lib.ptr(ref), _lib.ptr(ref_len), b,
        n, t, s, ws.data_ptr(), ws.numel() * 8, _lib.ptr(out.get("dref")),
        _lib.ptr(out.get("ops")), _lib.ptr(out.get("dpair")), _lib.stream_of(hyp)),
        "ob_nbest_edit_distance")
    return out


def nbest_oracle(dref: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``dref`` [B, N] of ``nbest_edit_distance`` -> (best_k int64 [B], dist int32 [B]): the live
    entry closest to the reference, ties to the smaller k; an utterance without a live entry gets
    best_k 0 and dist -1. Plain torch on ``dref``'s device."""
    n = dref.shape[1]
    live = dref >= 0
    # distance * N + k: the smallest key is the smallest distance, then the smallest k
    key = torch.where(live, dref.to(torch.int64) * n + torch.arange(n, device=dref.device),
                      torch.full_like(dref, torch.iinfo(torch.int64).max, dtype=torch.int64))
    best = key.min(dim=1).values
    some = live.any(dim=1)
    zero = torch.zeros_like(best)
    return (torch.where(some, best % n, zero),
            torch.where(some, best // n, zero - 1).to(torch.int32))


def check_mbr_scale(scale) -> float:
    scale = float(scale)
    if not 0 <= scale < math.inf:
        raise ValueError(f"mbr_scale must be >= 0 and finite, got {scale}")
    return scale


def mbr_select(hyp: torch.Tensor, hyp_len: torch.Tensor, n_hyp: torch.Tensor,
               scores: torch.Tensor, scale: float = 1.0):
    """Minimum-Bayes-risk selection from an n-best: hyp [B, N, T] / hyp_len [B, N] / n_hyp [B] and
    the entries' totals ``scores`` [B, N] (log domain). Over the live entries of an utterance,
    post_j = softmax(scale * scores)_j and risk_k = sum_j post_j * distance(entry k, entry j); the
    entry with the smallest risk wins, ties to the smaller k (``scale`` 0: uniform posterior; a
    large scale: the MAP entry).

    Returns (out int32 [B, T] padded with -1, cnt int32 [B], info) with info = {best_k int32 [B],
    risk float64 [B, N] (+inf for absent entries), post float64 [B, N] (0 for absent entries),
    dpair int32 [B, N, N]}. An utterance without a live entry returns the empty output and best_k
    0; one whose largest live score is -inf returns entry 0 with every risk +inf."""
    scale = check_mbr_scale(scale)
    hyp, hyp_len, n_hyp = _nbest_args("mbr_select", hyp, hyp_len, n_hyp)
    b, n, t = hyp.shape
    dev = hyp.device
    if scores.shape != (b, n):
        raise ValueError(f"mbr_select: scores {tuple(scores.shape)} do not match hyp "
                         f"{tuple(hyp.shape)}")
    sc = scores.to(device=dev, dtype=torch.float64).contiguous()
    dpair = nbest_edit_distance(hyp, hyp_len, n_hyp, pairwise=True)["dpair"]
    out = torch.empty((b, t), dtype=torch.int32, device=dev)
    cnt = torch.empty((b,), dtype=torch.int32, device=dev)
    best_k = torch.empty((b,), dtype=torch.int32, device=dev)
    risk = torch.empty((b, n), dtype=torch.float64, device=dev)
    post = torch.empty((b, n), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().ob_mbr_select(
        dpair.data_ptr(), hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(), sc.data_ptr(),
        scale, b, n, t, out.data_ptr(), cnt.data_ptr(), best_k.data_ptr(), risk.data_ptr(),
        post.data_ptr(), _lib.stream_of(hyp)), "ob_mbr_select")
    return out, cnt, {"best_k": best_k, "risk": risk, "post": post, "dpair": dpair}
