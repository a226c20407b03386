"""Phrase-list contextual biasing (hotword / phrase boosting) for the device beam searches
(csrc/bias.hip, csrc/ob_bias.h; the contracts are in include/onebit_hip.h).

``ContextBias(phrases, boost=1.0)``: ``phrases`` is a sequence of token-id sequences, or of
``(ids, boost)`` pairs; a phrase is 1..16 ids in 0..65534, its boost a float32 > 0 per token. The
same phrase given twice keeps the larger boost, and the same phrases in any order build the same
bytes. ``ContextBias.from_text(texts, encode, boost=1.0)`` runs the caller's ``encode`` (text -> the
model's token ids, offset included; no tokenizer is imported here) over ``texts``, which may also
hold ``(text, boost)`` pairs.

The automaton is built by the library's host builder (``ob_bias_build``): 16-byte node records
(fail link, has-children flag, phi, commit) and one open-addressed edge table. ``walk`` / ``bias`` /
``bias_fin`` run the kernels' own lookup routine on the host (``ob_bias_walk_host``); ``bias_step``
and ``bias_seq_score`` are the device scorers.

The rule: a hypothesis carries (state, kept). Extending by a token follows the trie edge if there
is one; otherwise the longest finished phrase on the way is committed into ``kept`` and matching
restarts at the root, or the match falls back along the fail links. A node without children
commits at once. ``bias(y) = kept + phi(state)`` counts the partial match, ``bias_fin(y) = kept +
commit(state)`` takes an unfinished one back. float64 sums of float32 values in a fixed order.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["ContextBias", "bias_step", "bias_seq_score", "MAX_PHRASE_LEN", "MAX_ID"]

MAX_PHRASE_LEN = 16
MAX_ID = 65534


def _is_pair(p) -> bool:
    return (isinstance(p, (tuple, list)) and len(p) == 2 and
            isinstance(p[0], (tuple, list, np.ndarray, torch.Tensor)) and
            not isinstance(p[1], (tuple, list, np.ndarray, torch.Tensor)))


class ContextBias:
    def __init__(self, phrases: Iterable, boost: float = 1.0):
        toks: List[int] = []
        lens: List[int] = []
        boosts: List[float] = []
        for p in phrases:
            ids, b = (p[0], p[1]) if _is_pair(p) else (p, boost)
            ids = [int(t) for t in (ids.tolist() if hasattr(ids, "tolist") else ids)]
            b = float(b)
            if not 1 <= len(ids) <= MAX_PHRASE_LEN:
                raise ValueError(f"a phrase has 1..{MAX_PHRASE_LEN} tokens, got {len(ids)}")
            if min(ids) < 0 or max(ids) > MAX_ID:
                raise ValueError(f"phrase {ids}: ids must be in 0..{MAX_ID}")
            with np.errstate(over="ignore"):
                b32 = float(np.float32(b))
            if not 0 < b32 < float("inf"):
                raise ValueError(f"phrase {ids}: the boost must be positive and finite, got {b}")
            toks += ids
            lens.append(len(ids))
            boosts.append(b32)
        self.n_phrases = len(lens)
        self._build(np.asarray(toks, np.int32), np.asarray(lens, np.int32),
                    np.asarray(boosts, np.float32))
        self._device: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}

    @classmethod
    def from_text(cls, texts: Iterable, encode: Callable[[str], Sequence[int]],
                  boost: float = 1.0) -> "ContextBias":
        phrases = []
        for t in texts:
            text, b = (t[0], t[1]) if isinstance(t, (tuple, list)) else (t, boost)
            phrases.append(([int(i) for i in encode(text)], b))
        return cls(phrases, boost)

    def _build(self, toks: np.ndarray, lens: np.ndarray, boosts: np.ndarray) -> None:
        lib = _lib.load()
        p = int(lens.shape[0])
        n_nodes, slots = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(lib.ob_bias_sizes(p, int(toks.shape[0]), ctypes.addressof(n_nodes),
                                     ctypes.addressof(slots)), "ob_bias_sizes")
        probe = ctypes.c_int32(0)
        while True:
            nodes = np.zeros((n_nodes.value, 4), np.int32)          # 16-byte records
            edges = np.zeros((slots.value, 2), np.uint64)           # 16-byte entries
            st = lib.ob_bias_build(toks.ctypes.data, lens.ctypes.data, boosts.ctypes.data, p,
                                   nodes.ctypes.data, nodes.nbytes, edges.ctypes.data,
                                   edges.nbytes, ctypes.addressof(n_nodes),
                                   ctypes.addressof(slots), ctypes.addressof(probe))
            if st == _lib.OB_OK:
                break
            if st == _lib.OB_ERR_SHAPE:
                raise ValueError("the phrase list is not valid")
            if n_nodes.value * 16 <= nodes.nbytes and slots.value * 16 <= edges.nbytes:
                _lib.check(st, "ob_bias_build")                     # (not the grow-and-retry status)
        self.n_nodes = int(n_nodes.value)
        self.slots = int(slots.value)
        self.max_probe = int(probe.value)
        self.nodes = np.ascontiguousarray(nodes[:self.n_nodes])
        self.edges = np.ascontiguousarray(edges[:self.slots])

    # ------------------------------------------------------------------------------------
    def walk_host(self, tokens, lens):
        """``ob_bias_walk_host``: tokens int32 [Q, T], lens int32 [Q] -> (state int32 [Q], kept,
        bias, bias_fin float64 [Q])."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        lens = np.ascontiguousarray(lens, np.int32)
        if tokens.ndim != 2 or lens.shape != (tokens.shape[0],):
            raise ValueError("walk_host: tokens [Q, T] and lens [Q] expected")
        q, t = tokens.shape
        state = np.zeros(q, np.int32)
        kept, bias, fin = (np.zeros(q, np.float64) for _ in range(3))
        _lib.check(_lib.load().ob_bias_walk_host(
            self.nodes.ctypes.data, self.n_nodes, self.edges.ctypes.data, self.slots,
            self.max_probe, tokens.ctypes.data, lens.ctypes.data, q, t, state.ctypes.data,
            kept.ctypes.data, bias.ctypes.data, fin.ctypes.data), "ob_bias_walk_host")
        return state, kept, bias, fin

    def walk(self, tokens: Sequence[int]) -> Tuple[int, float, float, float]:
        """(state, kept, bias, bias_fin) of one token sequence (host)."""
        toks = np.asarray([int(t) for t in tokens], np.int32).reshape(1, -1)
        st, kept, bias, fin = self.walk_host(toks, np.asarray([toks.shape[1]], np.int32))
        return int(st[0]), float(kept[0]), float(bias[0]), float(fin[0])

    def bias(self, tokens: Sequence[int]) -> float:
        """The running value: partial matches counted (host)."""
        return self.walk(tokens)[2]

    def bias_fin(self, tokens: Sequence[int]) -> float:
        """The closed value: an unfinished partial match taken back (host)."""
        return self.walk(tokens)[3]

    def device_tables(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(nodes, edges) on ``device`` (uploaded once per device; the upload cannot be captured, so
        a graph must have run the search once before its capture: GraphedInference's warm-up
        does)."""
        key = str(torch.device(device))
        if key not in self._device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ContextBias: run the decoder once outside the graph capture "
                                   "first (the tables are uploaded then)")
            self._device[key] = (torch.from_numpy(self.nodes.view(np.int64)).to(device),
                                 torch.from_numpy(self.edges.view(np.int64)).to(device))
        return self._device[key]

    def _args(self, device):
        nodes, edges = self.device_tables(device)
        return (nodes.data_ptr(), self.n_nodes, edges.data_ptr(), self.slots, self.max_probe)


def bias_step(bias: ContextBias, topi: torch.Tensor, tok: torch.Tensor, length: torch.Tensor,
              link: torch.Tensor, skip: torch.Tensor, st_in: torch.Tensor, st_out: torch.Tensor,
              kept_in: torch.Tensor, kept_out: torch.Tensor, bsc: torch.Tensor, n: int,
              eos: int = 2) -> torch.Tensor:
    """``ob_bias_step``: topi int32 [R, K], tok int64 [R], length int32 [R] or [B, N], link int32
    [R, 2], skip uint8 [R], st_in / st_out int32 [R] and kept_in / kept_out float64 [R] (the
    hypotheses' automaton states, two tables used alternately), bsc float64 [R, K] (written for
    rows with skip 0); ``n`` = beam slots per utterance."""
    if not topi.is_cuda:
        raise RuntimeError("bias_step runs on the HIP library (no CPU fallback)")
    rows, k = topi.shape
    lib = _lib.load()
    if not lib.ob_bias_supported(1, k, bias.n_nodes):
        raise ValueError(f"contextual bias: K={k} is not supported (1 <= K <= 32)")
    if n < 1 or rows % n or topi.dtype != torch.int32 or tok.shape != (rows,) or \
            tok.dtype != torch.int64 or length.numel() != rows or length.dtype != torch.int32 or \
            link.shape != (rows, 2) or skip.shape != (rows,) or st_in.shape != (rows,) or \
            st_out.shape != (rows,) or st_in.dtype != torch.int32 or \
            st_out.dtype != torch.int32 or kept_in.shape != (rows,) or \
            kept_out.shape != (rows,) or kept_in.dtype != torch.float64 or \
            kept_out.dtype != torch.float64 or bsc.shape != (rows, k) or \
            bsc.dtype != torch.float64:
        raise ValueError("bias_step: the arguments' shapes do not match")
    _lib.check(lib.ob_bias_step(*bias._args(topi.device), topi.data_ptr(), tok.data_ptr(),
                                length.data_ptr(), link.data_ptr(), skip.data_ptr(), rows // n, n,
                                k, int(eos), st_in.data_ptr(), st_out.data_ptr(),
                                kept_in.data_ptr(), kept_out.data_ptr(), bsc.data_ptr(),
                                _lib.stream_of(topi)), "ob_bias_step")
    return bsc


def bias_seq_score(bias: ContextBias, hyp: torch.Tensor, hyp_len: torch.Tensor) -> torch.Tensor:
    """``ob_bias_seq_score``: hyp int32 [..., T] padded with -1, hyp_len int32 [...] (< 0: an absent
    row) -> float64 [...], ``bias_fin`` of every hypothesis (-inf for absent rows)."""
    if not hyp.is_cuda:
        raise RuntimeError("bias_seq_score runs on the HIP library (no CPU fallback)")
    t = hyp.shape[-1]
    lead = hyp.shape[:-1]
    h = hyp.to(torch.int32).contiguous()
    ln = hyp_len.to(device=h.device, dtype=torch.int32).contiguous()
    if ln.shape != lead:
        raise ValueError(f"bias_seq_score: hyp {tuple(hyp.shape)} / hyp_len "
                         f"{tuple(hyp_len.shape)} do not match")
    out = torch.empty(lead, dtype=torch.float64, device=h.device)
    _lib.check(_lib.load().ob_bias_seq_score(*bias._args(h.device), h.data_ptr(), ln.data_ptr(),
                                             ln.numel(), t, out.data_ptr(), _lib.stream_of(h)),
               "ob_bias_seq_score")
    return out
