"""Back-off n-gram language model over the model's token ids, for shallow fusion in the device
decoders (csrc/ngram.hip, csrc/ob_ngram.h; the contracts are in include/onebit_hip.h).

``NGramLM(entries, order, unk_logp=None)``: ``entries`` maps an id tuple of length 1..order
(order <= 4, ids 0..65534) to ``(logp, backoff)`` in natural log; values are stored as float32.
``NGramLM.from_arpa(text_or_path, vocab=None, unk_logp=None)`` reads an ARPA file: log10 values
become natural log in float64 and are rounded to float32 once; without ``vocab`` the ARPA words are
decimal token ids, with it they go through the ``str -> id`` mapping (e.g. the pieces of a
``sentencepiece`` processor, which is not imported here); ``<s>`` is bos (1), ``</s>`` eos (2),
``<unk>`` supplies ``unk_logp`` (default ln 1e-10) and is no entry.

The table is built by the library's host builder (``ob_ngram_table_build``): one open-addressed
hash table of 16-byte entries, deterministic bytes, every entry within ``max_probe`` <= 64 slots
of its home. ``score`` / ``score_host`` run the kernels' own probe routine on the host;
``ngram_step`` and ``ngram_seq_logprob`` are the device scorers.

Scoring rule: the prefix is [bos] + tokens, the context h its last min(order - 1, len(prefix))
ids; for candidate w, from the longest context down: the first entry (h[-m:], w) ends the sum with
its logp, every context h[-m:] (m >= 1) that is an entry on the way adds its backoff, and a w
without a unigram ends it with unk_logp. float64 sum in that order.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["NGramLM", "ngram_step", "ngram_seq_logprob", "MAX_ORDER", "MAX_ID"]

MAX_ORDER = 4
MAX_ID = 65534
BOS, EOS = 1, 2
DEFAULT_UNK = math.log(1e-10)


def pack_keys(ids: np.ndarray, n: np.ndarray) -> np.ndarray:
    """ids int64 [E, 4] (n-gram w_1..w_n in columns 0..n-1), n [E] -> uint64 keys: four 16-bit
    fields of (id + 1), w_n in the lowest."""
    key = np.zeros(ids.shape[0], np.uint64)
    for j in range(MAX_ORDER):
        use = n > j                               # field j holds w_{n-j}
        col = np.where(use, ids[np.arange(ids.shape[0]), np.maximum(n - 1 - j, 0)] + 1, 0)
        key |= col.astype(np.uint64) << np.uint64(16 * j)
    return key


def pack_context(prefix: Sequence[int]) -> int:
    """The context state of a prefix that already starts with bos: its last three ids."""
    ctx = 0
    for t in list(prefix)[-3:]:
        ctx = ((ctx << 16) | (min(max(int(t), 0), MAX_ID) + 1)) & 0xFFFFFFFFFFFF
    return ctx


class NGramLM:
    bos, eos = BOS, EOS

    def __init__(self, entries: Mapping[Tuple[int, ...], Tuple[float, float]], order: int,
                 unk_logp: Optional[float] = None):
        order = int(order)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"order must be in 1..{MAX_ORDER}, got {order}")
        e = len(entries)
        ids = np.zeros((e, MAX_ORDER), np.int64)
        n = np.zeros(e, np.int64)
        vals = np.zeros((e, 2), np.float32)
        for i, (gram, (lp, bo)) in enumerate(entries.items()):
            gram = tuple(int(g) for g in gram)
            if not 1 <= len(gram) <= order:
                raise ValueError(f"n-gram {gram} has length {len(gram)}, order is {order}")
            if min(gram) < 0 or max(gram) > MAX_ID:
                raise ValueError(f"n-gram {gram}: ids must be in 0..{MAX_ID}")
            ids[i, :len(gram)] = gram
            n[i] = len(gram)
            vals[i] = (lp, bo)
        self._init_arrays(ids, n, vals, order, unk_logp)

    @classmethod
    def from_arrays(cls, ids, n, vals, order: int, unk_logp: Optional[float] = None) -> "NGramLM":
        """The constructor for large models: ids int [E, 4] (n-gram w_1..w_n in columns 0..n-1),
        n int [E] (1..order), vals float32 [E, 2] = (logp, backoff), without a Python dict."""
        ids = np.ascontiguousarray(ids, np.int64)
        n = np.ascontiguousarray(n, np.int64)
        vals = np.ascontiguousarray(vals, np.float32)
        order = int(order)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"order must be in 1..{MAX_ORDER}, got {order}")
        e = n.shape[0]
        if ids.shape != (e, MAX_ORDER) or vals.shape != (e, 2):
            raise ValueError("from_arrays: ids [E, 4], n [E], vals [E, 2] expected")
        used = np.arange(MAX_ORDER)[None, :] < n[:, None]
        if e and (n.min() < 1 or n.max() > order or ids[used].min() < 0 or
                  ids[used].max() > MAX_ID):
            raise ValueError(f"from_arrays: lengths must be in 1..{order}, ids in 0..{MAX_ID}")
        self = cls.__new__(cls)
        self._init_arrays(ids, n, vals, order, unk_logp)
        return self

    def _init_arrays(self, ids, n, vals, order, unk_logp) -> None:
        self.order = order
        self.n_entries = int(n.shape[0])
        self.unk_logp = float(np.float32(DEFAULT_UNK if unk_logp is None else unk_logp))
        self._build(pack_keys(ids, n), vals)
        self._device: Dict[str, torch.Tensor] = {}

    def _build(self, keys: np.ndarray, vals: np.ndarray) -> None:
        lib = _lib.load()
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.float32)
        n = keys.shape[0]
        slots = ctypes.c_int64(lib.ob_ngram_table_slots(n))
        if slots.value == 0:
            raise ValueError(f"{n} entries are not supported")
        probe = ctypes.c_int32(0)
        while True:
            table = np.zeros((slots.value, 2), np.uint64)       # 16-byte entries
            st = lib.ob_ngram_table_build(keys.ctypes.data, vals.ctypes.data, n, table.ctypes.data,
                                          table.nbytes, ctypes.addressof(slots),
                                          ctypes.addressof(probe))
            if st == _lib.OB_ERR_SHAPE:
                raise ValueError("the n-gram entries are not distinct")
            if st == _lib.OB_OK:
                break
            if slots.value * 16 <= table.nbytes:                # (not the grow-and-retry status)
                _lib.check(st, "ob_ngram_table_build")
        self.table = table
        self.slots = int(slots.value)
        self.max_probe = int(probe.value)

    # ------------------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, text_or_path, vocab: Optional[Mapping[str, int]] = None,
                  unk_logp: Optional[float] = None) -> "NGramLM":
        if isinstance(text_or_path, os.PathLike) or (isinstance(text_or_path, str) and
                                                     "\n" not in text_or_path):
            with open(text_or_path, "r", encoding="utf-8") as f:
                text = f.read()
        else:
            text = text_or_path
        ln10 = math.log(10.0)
        counts: Dict[int, int] = {}
        found: Dict[int, int] = {}
        entries: Dict[Tuple[int, ...], Tuple[float, float]] = {}
        arpa_unk = None
        section = None          # None before \data\, 0 inside it, n inside \n-grams:
        ended = False

        def word_id(word: str, where: str) -> Optional[int]:
            if word == "<s>":
                return BOS
            if word == "</s>":
                return EOS
            if word == "<unk>":
                return None
            if vocab is not None:
                if word not in vocab:
                    raise ValueError(f"{where}: word {word!r} is not in the vocabulary")
                wid = int(vocab[word])
            else:
                try:
                    wid = int(word)
                except ValueError:
                    raise ValueError(f"{where}: {word!r} is not a decimal token id") from None
            if not 0 <= wid <= MAX_ID:
                raise ValueError(f"{where}: token id {wid} is outside 0..{MAX_ID}")
            return wid

        for no, raw in enumerate(text.splitlines(), 1):
            line = raw.strip()
            where = f"ARPA line {no}"
            if not line or ended:
                continue
            if line == "\\data\\":
                section = 0
                continue
            if line == "\\end\\":
                ended = True
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                try:
                    section = int(line[1:-len("-grams:")])
                except ValueError:
                    raise ValueError(f"{where}: bad section header {line!r}") from None
                if section not in counts:
                    raise ValueError(f"{where}: section {line!r} was not declared in \\data\\")
                continue
            if section is None:
                continue                                   # text ahead of \data\
            if section == 0:
                if not line.startswith("ngram "):
                    raise ValueError(f"{where}: expected 'ngram N=count', got {line!r}")
                try:
                    n_s, c_s = line[len("ngram "):].split("=")
                    n_, c_ = int(n_s), int(c_s)
                except ValueError:
                    raise ValueError(f"{where}: expected 'ngram N=count', got {line!r}") from None
                if not 1 <= n_ <= MAX_ORDER:
                    raise ValueError(f"{where}: order {n_} is not supported (1..{MAX_ORDER})")
                counts[n_] = c_
                continue
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError(f"{where}: a {section}-gram needs {section + 1} or {section + 2} "
                                 f"fields, got {len(f)}")
            try:
                lp10 = float(f[0])
                bo10 = float(f[section + 1]) if len(f) == section + 2 else 0.0
            except ValueError:
                raise ValueError(f"{where}: bad number in {line!r}") from None
            found[section] = found.get(section, 0) + 1
            gram = [word_id(w, where) for w in f[1:section + 1]]
            lp = float(np.float32(np.float64(lp10) * ln10))
            bo = float(np.float32(np.float64(bo10) * ln10))
            if None in gram:                               # <unk>: no id, so no entry
                if section == 1:
                    arpa_unk = lp
                continue
            if tuple(gram) in entries:
                raise ValueError(f"{where}: n-gram {' '.join(f[1:section + 1])} occurs twice")
            entries[tuple(gram)] = (lp, bo)
        if not counts:
            raise ValueError("ARPA: no \\data\\ section with 'ngram N=count' lines")
        for n_, c_ in sorted(counts.items()):
            if found.get(n_, 0) != c_:
                raise ValueError(f"ARPA: \\data\\ declares {c_} {n_}-grams, the \\{n_}-grams: "
                                 f"section holds {found.get(n_, 0)}")
        if unk_logp is None:
            unk_logp = arpa_unk
        return cls(entries, max(counts), unk_logp)

    # ------------------------------------------------------------------------------------
    def context(self, tokens: Sequence[int]) -> int:
        """The packed context state of the prefix [bos] + tokens."""
        return pack_context([self.bos] + [int(t) for t in tokens])

    def score_host(self, ctx, w, vocab_size: int = MAX_ID + 1, probes: bool = False):
        """The scoring rule on the host through the kernels' probe routine
        (``ob_ngram_score_host``): ctx uint64 [Q] packed contexts, w int32 [Q] -> float64 [Q]
        (and the table slots examined per query with ``probes=True``)."""
        ctx = np.ascontiguousarray(ctx, np.uint64)
        w = np.ascontiguousarray(w, np.int32)
        if ctx.shape != w.shape or ctx.ndim != 1:
            raise ValueError("score_host: ctx and w must be 1-D arrays of one length")
        out = np.empty(ctx.shape[0], np.float64)
        pr = np.zeros(ctx.shape[0], np.int32)
        _lib.check(_lib.load().ob_ngram_score_host(
            self.table.ctypes.data, self.slots, self.max_probe, self.order, int(vocab_size),
            self.unk_logp, ctx.ctypes.data, w.ctypes.data, ctx.shape[0], out.ctypes.data,
            pr.ctypes.data), "ob_ngram_score_host")
        return (out, pr) if probes else out

    def score(self, tokens: Sequence[int], w: int) -> float:
        """log P(w | [bos] + tokens) by the rule (host)."""
        return float(self.score_host(np.array([self.context(tokens)], np.uint64),
                                     np.array([w], np.int32))[0])

    def seq_logprob(self, tokens: Sequence[int]) -> float:
        """The sum over the tokens and the closing eos, ascending position (host)."""
        toks = [int(t) for t in tokens]
        total = 0.0
        for j, w in enumerate(toks + [self.eos]):
            total += self.score(toks[:j], w)
        return total

    def device_table(self, device) -> torch.Tensor:
        """The table on ``device`` (uploaded once per device; the upload cannot be captured, so a
        graph must have run the search once before its capture: GraphedInference's warm-up does)."""
        key = str(torch.device(device))
        if key not in self._device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("NGramLM: run the decoder once outside the graph capture first "
                                   "(the table is uploaded then)")
            self._device[key] = torch.from_numpy(self.table.view(np.int64)).to(device)
        return self._device[key]

    def _args(self, device, vocab_size: int):
        return (self.device_table(device).data_ptr(), self.slots, self.max_probe, self.order,
                int(vocab_size), self.unk_logp)


def ngram_step(lm: NGramLM, topi: torch.Tensor, tok: torch.Tensor, length: torch.Tensor,
               link: torch.Tensor, skip: torch.Tensor, ctx_in: torch.Tensor,
               ctx_out: torch.Tensor, lmsc: torch.Tensor, n: int,
               vocab_size: int = MAX_ID + 1) -> torch.Tensor:
    """``ob_ngram_step``: topi int32 [R, K], tok int64 [R], length int32 [R] or [B, N], link int32
    [R, 2], skip uint8 [R], ctx_in / ctx_out int64 [R] (the packed contexts, two tables used
    alternately), lmsc float64 [R, K] (written for rows with skip 0); ``n`` = beam slots per
    utterance."""
    if not topi.is_cuda:
        raise RuntimeError("ngram_step runs on the HIP library (no CPU fallback)")
    rows, k = topi.shape
    lib = _lib.load()
    if not lib.ob_ngram_supported(lm.order, int(vocab_size), k):
        raise ValueError(f"n-gram LM: order={lm.order}, V={vocab_size}, K={k} is not supported "
                         "(1 <= order <= 4, V <= 65535, 1 <= K <= 32)")
    if n < 1 or rows % n or topi.dtype != torch.int32 or tok.shape != (rows,) or \
            tok.dtype != torch.int64 or length.numel() != rows or length.dtype != torch.int32 or \
            link.shape != (rows, 2) or skip.shape != (rows,) or ctx_in.shape != (rows,) or \
            ctx_out.shape != (rows,) or ctx_in.dtype != torch.int64 or \
            ctx_out.dtype != torch.int64 or lmsc.shape != (rows, k) or lmsc.dtype != torch.float64:
        raise ValueError("ngram_step: the arguments' shapes do not match")
    _lib.check(lib.ob_ngram_step(*lm._args(topi.device, vocab_size), topi.data_ptr(),
                                 tok.data_ptr(), length.data_ptr(), link.data_ptr(),
                                 skip.data_ptr(), rows // n, n, k, lm.bos, ctx_in.data_ptr(),
                                 ctx_out.data_ptr(), lmsc.data_ptr(), _lib.stream_of(topi)),
               "ob_ngram_step")
    return lmsc


def ngram_seq_logprob(lm: NGramLM, hyp: torch.Tensor, hyp_len: torch.Tensor,
                      vocab_size: int = MAX_ID + 1, per_token: bool = False):
    """``ob_ngram_seq_logprob``: hyp int32 [..., T] padded with -1, hyp_len int32 [...] (< 0: an
    absent row) -> float64 [...], the LM score of every hypothesis with its closing eos (-inf for
    absent rows); with ``per_token`` also float64 [..., T + 1], the per-position scores."""
    if not hyp.is_cuda:
        raise RuntimeError("ngram_seq_logprob runs on the HIP library (no CPU fallback)")
    t = hyp.shape[-1]
    lead = hyp.shape[:-1]
    h = hyp.to(torch.int32).contiguous()
    ln = hyp_len.to(device=h.device, dtype=torch.int32).contiguous()
    if ln.shape != lead:
        raise ValueError(f"ngram_seq_logprob: hyp {tuple(hyp.shape)} / hyp_len "
                         f"{tuple(hyp_len.shape)} do not match")
    rows = ln.numel()
    out = torch.empty(lead, dtype=torch.float64, device=h.device)
    tok_lm = torch.empty(lead + (t + 1,), dtype=torch.float64, device=h.device) if per_token \
        else None
    _lib.check(_lib.load().ob_ngram_seq_logprob(*lm._args(h.device, vocab_size), h.data_ptr(),
                                                ln.data_ptr(), rows, t, lm.bos, lm.eos,
                                                out.data_ptr(), _lib.ptr(tok_lm),
                                                _lib.stream_of(h)), "ob_ngram_seq_logprob")
    return (out, tok_lm) if per_token else out
