"""Autoregressive beam search with the attention decoder (``decoder="attention"``): KV-cached,
static shapes, no host synchronisation, capturable in the inference HIP graph
(csrc/attdec.hip).

Per utterance N beam slots; before step 0 only slot 0 is live (score 0, empty prefix). Step t:
every live, unfinished slot r gets ``lp_r = log_softmax(out(ln(y_r,t)))`` over the full
vocabulary, pad / bos / blank are removed from the candidates afterwards, and candidate (r, v)
scores ``s_r + lp_r[v]`` in float64; a finished slot (one that emitted eos) competes as itself,
unchanged. The N candidates with the largest key ``score / max(n, 1) ** length_penalty`` (n =
emitted tokens, eos counted) survive, ties to the smaller slot, then the smaller token. After
``max_len`` steps the slots are the n-best, best key first; a hypothesis that is not finished was
truncated at ``max_len`` tokens.

Data flow of a step: embedding -> per layer [packed q|k|v projection, ``ob_decattn_step`` (appends
the row's K/V to the cache and attends its own ancestry through the ``anc`` table), grouped
cross-attention on the K/V projected once per utterance, FFN] -> ``ob_seq_topk`` (log-sum-exp +
the N best ids per row, no [R, V] logits) -> ``ob_attdec_beam_step`` (selection, next inputs, the
new ``anc`` rows). A beam reorder rewrites ``anc`` only; cached K/V never move.

``joint_beam_search`` is the one-pass joint CTC/attention decode (csrc/ctcprefix.hip): the same
search with S = (1 - w) * A + w * C in place of the score, A the attention sum above and C the
CTC prefix score log P_ctc(the transcript starts with the prefix | audio), for eos
log P_ctc(prefix | audio). Every live slot offers its K = ``ctc_cand`` best attention candidates
(the pre-beam), ``ob_ctc_prefix_step`` scores them all in one launch from the one stored CTC
state per slot, candidates CTC cannot align (C = -inf) are dropped, and
``ob_attdec_joint_step`` keeps the N best keys S / norm[n]. eos is a candidate only when it is
among a slot's K attention candidates; an utterance can end with fewer than N live slots, or
with none (``n_hyp`` 0) when every candidate of every live slot is CTC-impossible and none has
finished, e.g. more tokens than frames.

All of it is one loop, ``_BeamSearch``: per step ``propose`` (decoder + ``ob_seq_topk``),
``score_ctc`` (``ob_ctc_prefix_step``), ``score_lm`` (``ob_ngram_step``) and ``select`` (the beam
step), then ``finish``. The public functions check their arguments and run it; ``_search_mode``
is the rule for what a call runs:

====================================  ========  ========================  ======================
call                                  K         beam step                 info beyond the four
====================================  ========  ========================  ======================
``attention_beam_search``             N         ``ob_attdec_beam_step``   --
``joint_beam_search``, w > 0, no LM   ctc_cand  ``ob_attdec_joint_step``  att, ctc
``joint_beam_search``, w == 0, no LM  ctc_cand  ``ob_attdec_beam_step``   att (= score), ctc (0)
``joint_beam_search``, LM, lw > 0     ctc_cand  ``ob_attdec_fused_step``  att, ctc, lm
====================================  ========  ========================  ======================

The CTC scorer runs when w > 0 (with the LM and w == 0 the fused step gets no ``cpsi``), the LM
scorer when there is an LM with ``lm_weight`` > 0. A search allocates only its mode's buffers.
"""
from __future__ import annotations

import ctypes
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib

__all__ = ["attention_beam_search", "joint_beam_search", "ctc_frame_lse", "ctc_prefix_step",
           "decattn_step", "seq_topk", "SPECIAL"]

SPECIAL = {"pad": 0, "bos": 1, "eos": 2, "blank": 3}  # the project's token ids
MAX_BEAM = 32      # ob_attdec_supported
MAX_BANNED = 8     # ob_seq_topk


def decattn_step(qkv: torch.Tensor, cache: torch.Tensor, anc: torch.Tensor,
                 skip: Optional[torch.Tensor], heads: int, t: int) -> torch.Tensor:
    """``ob_decattn_step``: qkv [R, 3e] (q | k | v of position t), cache [L, R, 2e] (one layer's),
    anc int32 [R, L], skip uint8 [R] or None -> ctx [R, e]; stores the rows' K/V at position t."""
    if not qkv.is_cuda:
        raise RuntimeError("decattn_step runs on the HIP library (no CPU fallback)")
    qkv = qkv.contiguous()
    rows, w = qkv.shape
    e = w // 3
    L = cache.shape[0]
    if cache.shape != (L, rows, 2 * e) or not cache.is_contiguous() or anc.shape != (rows, L) \
            or anc.dtype != torch.int32 or not anc.is_contiguous() or e % heads:
        raise ValueError(f"decattn_step: qkv {tuple(qkv.shape)}, cache {tuple(cache.shape)}, anc "
                         f"{tuple(anc.shape)} do not match")
    ctx = torch.empty((rows, e), dtype=torch.float32, device=qkv.device)
    _lib.check(_lib.load().ob_decattn_step(qkv.data_ptr(), w, cache.data_ptr(), anc.data_ptr(),
                                           _lib.ptr(skip), rows, heads, e // heads, L, int(t),
                                           ctx.data_ptr(), _lib.stream_of(qkv)),
               "ob_decattn_step")
    return ctx


def _banned_array(banned: Sequence[int]):
    ids = sorted({int(i) for i in banned})
    if len(ids) > MAX_BANNED:
        raise ValueError(f"at most {MAX_BANNED} banned ids, got {len(ids)}")
    return (ctypes.c_int32 * max(len(ids), 1))(*ids), len(ids)


def seq_topk(hidden: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], k: int,
             banned: Sequence[int] = (), skip: Optional[torch.Tensor] = None, out=None):
    """``ob_seq_topk``: hidden [R, d] fp32, weight [V, d], bias [V] or None -> (lse float64 [R],
    the log-sum-exp of ``hidden @ weight.T + bias`` over all V; topv float32 [R, k]; topi int32
    [R, k]): the k largest logits among the ids not in ``banned`` (value descending, ties to the
    smaller id, padded with (-inf, -1)). Rows with ``skip[r] != 0`` (uint8) are not computed and
    keep what ``out`` = (lse, topv, topi) held. The [R, V] logits never exist."""
    if not hidden.is_cuda:
        raise RuntimeError("seq_topk runs on the HIP library (no CPU fallback)")
    h = hidden.contiguous().float()
    w = weight.detach().contiguous().float()
    bs = bias.detach().contiguous().float() if bias is not None else None
    r, d = h.shape
    v = w.shape[0]
    if w.shape[1] != d or (bs is not None and bs.shape != (v,)) or \
            (skip is not None and (skip.shape != (r,) or skip.dtype != torch.uint8)):
        raise ValueError(f"seq_topk: hidden {tuple(h.shape)}, weight {tuple(w.shape)} do not match")
    lib = _lib.load()
    need = lib.ob_seq_topk_workspace(r, d, v, k)
    if need == 0 and (r > 0 or lib.ob_seq_topk_workspace(1, d, v, k) == 0):
        raise ValueError(f"seq_topk: shape R={r} d={d} V={v} K={k} is not supported "
                         "(d % 16 == 0, 16 <= d <= 256, 1 <= K <= 32)")
    arr, nb = _banned_array(banned)
    ws = torch.empty((max(need, 8) // 8,), dtype=torch.int64, device=h.device)
    if out is None:
        out = (torch.empty((r,), dtype=torch.float64, device=h.device),
               torch.empty((r, k), dtype=torch.float32, device=h.device),
               torch.empty((r, k), dtype=torch.int32, device=h.device))
    lse, topv, topi = out
    _lib.check(lib.ob_seq_topk(h.data_ptr(), r, d, w.data_ptr(), _lib.ptr(bs), v,
                               ctypes.addressof(arr), nb, _lib.ptr(skip), k, ws.data_ptr(),
                               ws.numel() * 8, lse.data_ptr(), topv.data_ptr(), topi.data_ptr(),
                               _lib.stream_of(h)), "ob_seq_topk")
    return lse, topv, topi


def length_norm(max_len: int, length_penalty: float) -> torch.Tensor:
    """norm[n] = max(n, 1) ** length_penalty for n = 0..max_len, float64 on the host."""
    return torch.tensor([float(max(n, 1)) ** float(length_penalty) for n in range(max_len + 1)],
                        dtype=torch.float64)


_NORM: Dict[tuple, torch.Tensor] = {}


def _norm_on_device(dev: torch.device, max_len: int, length_penalty: float) -> torch.Tensor:
    """The host table uploaded once per (device, max_len, length_penalty). The upload is a copy
    from pageable host memory, which a stream capture cannot record: a graph must have run the
    same search once before it is captured (GraphedInference's warm-up does)."""
    key = (str(dev), int(max_len), float(length_penalty))
    if key not in _NORM:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("attention_beam_search: run the search once outside the graph "
                               "capture first (the length-normaliser table is uploaded then)")
        _NORM[key] = length_norm(max_len, length_penalty).to(dev)
    return _NORM[key]


@torch.no_grad()
def attention_beam_search(model, enc: torch.Tensor, mask: torch.Tensor, beam_size: int = 10,
                          max_len: int = 64, length_penalty: float = 0.0,
                          special: Optional[Dict[str, int]] = None):
    """Batched beam search with ``model.decoder`` on the encoder output ``enc`` [B, T', d] /
    ``mask`` [B, T'] (module docstring); ``beam_size`` 1 is greedy decoding.

    Returns (hyp int32 [B, N, max_len] padded with -1, hyp_len int32 [B, N], n_hyp int32 [B],
    score float64 [B, N] -- the sum of log-probabilities, -inf for dead slots -- and info =
    {finished bool [B, N], trace_parent / trace_token int32 [max_len, B, N], trace_score float64
    [max_len, B, N]}), best key first: the n-best layout of ``ctc_beam_search_nbest_device``.
    An utterance whose mask has no valid frame has ``n_hyp`` 0. ``trace_token``: -1 = a finished
    slot carried over, -2 = a dead slot. ``special``: token ids, default ``{"pad": 0, "bos": 1,
    "eos": 2, "blank": 3}``. No host synchronisation; fixed shapes: capturable in a HIP graph."""
    if not enc.is_cuda:
        raise RuntimeError("attention_beam_search runs on the HIP library (no CPU fallback)")
    ids = dict(SPECIAL, **(special or {}))
    _, lk, d = enc.shape
    n, L = int(beam_size), int(max_len)
    heads = model.decoder.dec.layers[0].self_attn.num_heads
    if not _lib.load().ob_attdec_supported(n, d, heads, lk, L):
        raise ValueError(f"attention beam search: beam_size={n}, d={d}, heads={heads}, T'={lk}, "
                         f"max_len={L} is not supported (1 <= beam_size <= {MAX_BEAM}, d % 16 == 0,"
                         " d <= 256, d / heads in {16, 32, 36, 64}, 1 <= max_len <= 255, T' <= 256)")
    return _BeamSearch(model, enc, mask, n, None, L, length_penalty, ids).run()


def ctc_frame_lse(logits: torch.Tensor, lens: torch.Tensor, out: Optional[torch.Tensor] = None):
    """``ob_ctc_frame_lse``: CTC logits [B, T', V] fp32, lens [B] -> flse float64 [B, T'], the
    log-sum-exp of every frame t < lens[b]; later frames keep what ``out`` held."""
    if not logits.is_cuda:
        raise RuntimeError("ctc_frame_lse runs on the HIP library (no CPU fallback)")
    x = logits.contiguous().float()
    b, tp, v = x.shape
    ln = lens.to(device=x.device, dtype=torch.int64).contiguous()
    if tp < 1 or tp > 256 or v < 1 or ln.shape != (b,):
        raise ValueError(f"ctc_frame_lse: logits {tuple(x.shape)}, lens {tuple(ln.shape)} is not "
                         "supported (1 <= T' <= 256)")
    if out is None:
        out = torch.empty((b, tp), dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().ob_ctc_frame_lse(x.data_ptr(), ln.data_ptr(), b, tp, v, out.data_ptr(),
                                            _lib.stream_of(x)), "ob_ctc_frame_lse")
    return out


def ctc_prefix_state(b: int, n: int, k: int, tp: int, device) -> torch.Tensor:
    """The scorer's two state tables, float64 [2, B * N, T', 2] (``ob_ctc_prefix_workspace``
    bytes: independent of K)."""
    need = _lib.load().ob_ctc_prefix_workspace(b, n, k, tp)
    if need == 0 and b > 0:
        raise ValueError(f"CTC prefix scorer: N={n}, K={k}, T'={tp} is not supported "
                         "(1 <= N <= K <= 32, 1 <= T' <= 256)")
    assert need == 2 * b * n * tp * 2 * 8
    return torch.empty((2, b * n, tp, 2), dtype=torch.float64, device=device)


def ctc_prefix_step(logits: torch.Tensor, flse: torch.Tensor, lens: torch.Tensor,
                    topi: torch.Tensor, tok: torch.Tensor, length: torch.Tensor,
                    link: torch.Tensor, skip: torch.Tensor, state_in: torch.Tensor,
                    state_out: torch.Tensor, cpsi: torch.Tensor, blank: int = SPECIAL["blank"],
                    eos: int = SPECIAL["eos"]) -> torch.Tensor:
    """``ob_ctc_prefix_step``: logits [B, T', V] fp32, flse float64 [B, T'], lens int64 [B], topi
    int32 [R, K], tok int64 [R], length int32 [R] or [B, N], link int32 [R, 2], skip uint8 [R],
    state_in / state_out float64 [R, T', 2], cpsi float64 [R, K] (written for rows with skip 0)."""
    if not logits.is_cuda:
        raise RuntimeError("ctc_prefix_step runs on the HIP library (no CPU fallback)")
    b, tp, v = logits.shape
    rows, k = topi.shape
    n = rows // max(b, 1)
    if b * n != rows or logits.dtype != torch.float32 or not logits.is_contiguous() or \
            flse.shape != (b, tp) or lens.dtype != torch.int64 or lens.shape != (b,) or \
            tok.shape != (rows,) or length.numel() != rows or link.shape != (rows, 2) or \
            skip.shape != (rows,) or state_in.shape != (rows, tp, 2) or \
            state_out.shape != (rows, tp, 2) or cpsi.shape != (rows, k):
        raise ValueError("ctc_prefix_step: the arguments' shapes do not match")
    _lib.check(_lib.load().ob_ctc_prefix_step(
        logits.data_ptr(), flse.data_ptr(), lens.data_ptr(), topi.data_ptr(), tok.data_ptr(),
        length.data_ptr(), link.data_ptr(), skip.data_ptr(), b, n, k, tp, v, int(blank), int(eos),
        state_in.data_ptr(), state_out.data_ptr(), cpsi.data_ptr(), _lib.stream_of(logits)),
        "ob_ctc_prefix_step")
    return cpsi


@torch.no_grad()
def joint_beam_search(model, enc: torch.Tensor, mask: torch.Tensor, ctc_logits: torch.Tensor,
                      beam_size: int = 10, max_len: int = 64, ctc_weight: float = 0.3,
                      ctc_cand: Optional[int] = None, length_penalty: float = 0.0,
                      special: Optional[Dict[str, int]] = None, lm=None, lm_weight: float = 0.0,
                      bias=None, bias_weight: float = 0.0):
    """One-pass joint CTC/attention beam search (module docstring) on the encoder output ``enc``
    [B, T', d] / ``mask`` [B, T'] and the CTC head's logits ``ctc_logits`` [B, T', V] of the same
    frames. ``ctc_weight`` w in [0, 1]; ``ctc_cand`` K, the attention candidates a slot offers per
    step, ``beam_size`` <= K <= 32, default min(32, 2 * beam_size).

    Returns ``attention_beam_search``'s tuple with ``score`` = S = (1 - w) * A + w * C and info
    additionally holding ``att`` (A) and ``ctc`` (C), float64 [B, N], in the same order (-inf for
    dead slots). With w == 0 the CTC scorer does not run, nothing is dropped and S = A exactly
    (``ctc`` is 0). No host synchronisation; fixed shapes: capturable in a HIP graph.

    ``lm`` (an ``ngram.NGramLM``) with ``lm_weight`` > 0 adds shallow fusion: every step
    ``ob_ngram_step`` scores the same [R, K] candidates from one stored context per slot and
    ``ob_attdec_fused_step`` keeps the N best keys of S = ((1 - w) * A + w * C) + lm_weight * Lm,
    Lm the LM score of the prefix (with eos once finished); info then also holds ``lm``. With
    w == 0 the CTC scorer does not run: attention + LM only. ``lm=None`` or ``lm_weight == 0`` is
    the search without an LM, unchanged.

    ``bias`` (a ``bias.ContextBias``) with ``bias_weight`` > 0 adds phrase-list contextual biasing:
    every step ``ob_bias_step`` scores the candidates from one stored automaton state per slot and
    ``ob_attdec_biased_step`` keeps the N best keys of S = (((1 - w) * A + w * C) + lm_weight * Lm)
    + bias_weight * Bi, Bi the running bias(y) of the prefix (bias_fin(y) once finished); info then
    also holds ``bias``. It combines with any ``ctc_weight`` and with or without an LM.
    ``bias=None`` or ``bias_weight == 0`` is the search without it, unchanged."""
    if not enc.is_cuda or not ctc_logits.is_cuda:
        raise RuntimeError("joint_beam_search runs on the HIP library (no CPU fallback)")
    ids = dict(SPECIAL, **(special or {}))
    w = float(ctc_weight)
    if not 0.0 <= w <= 1.0:
        raise ValueError(f"ctc_weight must be in [0, 1], got {ctc_weight}")
    if lm_weight < 0 or lm_weight != lm_weight:
        raise ValueError(f"lm_weight must be >= 0, got {lm_weight}")
    bias_weight = float(bias_weight)
    if not 0 <= bias_weight < float("inf"):
        raise ValueError(f"bias_weight must be >= 0 and finite, got {bias_weight}")
    if bias_weight != 0 and bias is None:
        raise ValueError("bias_weight is set but bias is None")
    use_bias = bias is not None and bias_weight != 0
    dec = model.decoder
    b, lk, d = enc.shape
    n, L = int(beam_size), int(max_len)
    mode = _search_mode(n, ctc_cand, True, w, lm, lm_weight)
    k = mode.k
    heads = dec.dec.layers[0].self_attn.num_heads
    lib = _lib.load()
    if not lib.ob_attdec_supported(n, d, heads, lk, L) or not lib.ob_ctc_prefix_supported(n, k, lk):
        raise ValueError(f"joint beam search: beam_size={n}, ctc_cand={k}, d={d}, heads={heads}, "
                         f"T'={lk}, max_len={L} is not supported (1 <= beam_size <= ctc_cand <= "
                         f"{MAX_BEAM}, d % 16 == 0, d <= 256, d / heads in {{16, 32, 36, 64}}, "
                         "1 <= max_len <= 255, 1 <= T' <= 256)")
    if ctc_logits.dim() != 3 or ctc_logits.shape[:2] != (b, lk) or mask.shape != (b, lk):
        raise ValueError(f"joint beam search: ctc_logits {tuple(ctc_logits.shape)} / mask "
                         f"{tuple(mask.shape)} do not match enc {tuple(enc.shape)}")
    if mode.lm:
        v = dec.out.weight.shape[0]
        if not lib.ob_ngram_supported(lm.order, v, k):
            raise ValueError(f"joint beam search: an n-gram LM of order {lm.order} at V={v}, "
                             f"ctc_cand={k} is not supported (order <= 4, V <= 65535)")
        if (ids["bos"], ids["eos"]) != (lm.bos, lm.eos):
            raise ValueError(f"joint beam search: the LM's bos / eos are {lm.bos} / {lm.eos}, the "
                             f"search's {ids['bos']} / {ids['eos']}")
    if use_bias and not lib.ob_bias_supported(dec.out.weight.shape[0], k, bias.n_nodes):
        raise ValueError(f"joint beam search: a bias at V={dec.out.weight.shape[0]}, ctc_cand={k} "
                         "is not supported (V <= 65535)")
    return _BeamSearch(model, enc, mask, n, ctc_cand, L, length_penalty, ids, ctc_logits, w, lm,
                       lm_weight, bias if use_bias else None, bias_weight).run()


class _SearchMode(NamedTuple):
    """What one search runs (``_search_mode``)."""
    entry: str               # the C entry of the beam step
    k: int                   # candidates a slot offers per step
    ctc: bool                # ob_ctc_prefix_step runs every step
    lm: bool                 # ob_ngram_step runs every step
    info: Tuple[str, ...]    # info's keys beyond the four of attention_beam_search


def _search_mode(beam_size: int, cand: Optional[int], joint: bool, ctc_weight: float = 0.0,
                 lm=None, lm_weight: float = 0.0) -> _SearchMode:
    """The mode rule of the one loop. ``joint`` False is ``attention_beam_search`` (K = N, the
    plain beam step); True is ``joint_beam_search`` with K = ``cand`` (default min(32, 2 N)):
    the fused step with an LM and ``lm_weight`` > 0 (the CTC scorer runs only when w > 0), else
    the joint step when w > 0, else the plain beam step on the K candidates (no scorer runs)."""
    if not joint:
        return _SearchMode("ob_attdec_beam_step", int(beam_size), False, False, ())
    k = min(32, 2 * int(beam_size)) if cand is None else int(cand)
    if lm is not None and lm_weight > 0:
        return _SearchMode("ob_attdec_fused_step", k, ctc_weight > 0, True, ("att", "ctc", "lm"))
    if ctc_weight > 0:
        return _SearchMode("ob_attdec_joint_step", k, True, False, ("att", "ctc"))
    return _SearchMode("ob_attdec_beam_step", k, False, False, ("att", "ctc"))


# the slots' score terms a step entry takes besides ``score``
_STEP_TERMS = {"ob_attdec_beam_step": (), "ob_attdec_joint_step": ("att", "ctc"),
               "ob_attdec_fused_step": ("att", "ctc", "lm")}
BIASED_STEP = "ob_attdec_biased_step"   # the fused step with the bias term; the LM is optional


def _clone(x):
    if isinstance(x, torch.Tensor):
        return x.clone()
    if isinstance(x, dict):
        return {key: _clone(v) for key, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_clone(v) for v in x)
    return x


class _BeamSearch:
    """The one beam-search loop behind ``attention_beam_search`` and ``joint_beam_search`` (their
    docstrings; the arguments are theirs, already checked; ``ctc_logits`` None = the attention
    search). ``mode`` (``_search_mode``) says which scorers run and which C entry selects.

    ``state`` is every buffer a step reads or writes, by name: score, att / ctc / lm (the slots'
    terms, joint / LM only), length, fin, tok, skip, link (joint only), anc [2, R, L] (the two
    ancestry tables, used alternately), trace (parent, token, score), cand (lse, topv, topi),
    cpsi and ctc_state [2, R, T', 2] (CTC scorer only), lmctx [2, R] and lmsc (LM only), bst
    [2, R], bkept [2, R], bsc and the slot term bias (bias only), norm and cache (the decoder's). ``hidden`` is the last ``propose``'s decoder output [R, d].

    A step is ``propose(t)``, ``score_ctc(t)`` if ``mode.ctc``, ``score_lm(t)`` if ``mode.lm``,
    ``score_bias(t)`` if ``self.bias`` is set (the search then selects with
    ``ob_attdec_biased_step`` whatever ``mode.entry`` says: the mode tuple knows no bias),
    ``select(t)``; ``finish()`` after the last returns the public functions' tuple; ``run()`` does
    all of it. The scorers only rewrite cand-sized scratch and the table of step t + 1, so any of
    the first three phases can be repeated at its step; ``select`` advances the slots, and
    ``select(t, clone_state(...))`` runs it on copies instead."""

    def __init__(self, model, enc, mask, beam_size, cand, max_len, length_penalty, ids,
                 ctc_logits=None, ctc_weight=0.0, lm=None, lm_weight=0.0, bias=None,
                 bias_weight=0.0):
        joint = ctc_logits is not None
        self.bias = bias if joint and bias is not None and bias_weight != 0 else None
        self.bw = float(bias_weight)
        mode = self.mode = _search_mode(beam_size, cand, joint, ctc_weight, lm, lm_weight)
        dec = self.dec = model.decoder
        b, lk, _ = enc.shape
        n, k, L = int(beam_size), mode.k, int(max_len)
        self.b, self.n, self.L, self.ids = b, n, L, ids
        self.w, self.lm, self.lw = float(ctc_weight), lm, float(lm_weight)
        self.banned = (ids["pad"], ids["bos"], ids["blank"])
        dev = enc.device
        rows = b * n
        enc = enc.contiguous().float()
        if joint:
            self.z = ctc_logits.contiguous().float()
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8

        def new(shape, dtype, make=torch.empty):
            return make(shape, dtype=dtype, device=dev)

        # att, ctc, lm, link and lmctx start at zero; the rest is written before it is read
        s = self.state = {"score": new((b, n), f64)}
        if joint:
            s["att"], s["ctc"] = new((b, n), f64, torch.zeros), new((b, n), f64, torch.zeros)
        if mode.lm:
            s["lm"] = new((b, n), f64, torch.zeros)
        s.update(length=new((b, n), i32), fin=new((b, n), u8), tok=new((rows,), torch.int64),
                 skip=new((rows,), u8))
        if joint:
            s["link"] = new((rows, 2), i32, torch.zeros)
        s["anc"] = new((2, rows, L), i32)
        s["trace"] = (new((L, b, n), i32), new((L, b, n), i32), new((L, b, n), f64))
        self.hyp = new((b, n, L), i32)
        self.hyp_len, self.n_hyp = new((b, n), i32), new((b,), i32)
        self.score_out, self.finished = new((b, n), f64), new((b, n), u8)
        # what finish() reports beyond the four entries of attention_beam_search
        self.info_keys = mode.info + (("bias",) if self.bias is not None else ())
        if self.bias is not None:
            s["bias"] = new((b, n), f64, torch.zeros)
        self.info = {"finished": self.finished.view(torch.bool), "trace_parent": s["trace"][0],
                     "trace_token": s["trace"][1], "trace_score": s["trace"][2],
                     **{key: new((b, n), f64) for key in self.info_keys}}
        if b == 0:
            return
        s["norm"] = _norm_on_device(dev, L, length_penalty)
        if mode.lm:
            lm.device_table(dev)                  # (uploaded on first use, outside any capture)
        self.stream = _lib.stream_of(enc)
        s["cache"] = dec.new_cache(enc, mask, n, L)
        _lib.check(_lib.load().ob_attdec_init(
            s["cache"]["kmask"].data_ptr(), b, n, lk, L, ids["bos"], s["score"].data_ptr(),
            s["length"].data_ptr(), s["fin"].data_ptr(), s["tok"].data_ptr(),
            s["skip"].data_ptr(), s["anc"][0].data_ptr(), self.stream), "ob_attdec_init")
        # the rows' candidates of a step; a skipped row's entries are never read by the beam step
        s["cand"] = (new((rows,), f64), new((rows, k), torch.float32), new((rows, k), i32))
        if mode.lm:
            s["lmctx"] = new((2, rows), torch.int64, torch.zeros)
            s["lmsc"] = new((rows, k), f64)
        if self.bias is not None:
            self.bias.device_tables(dev)          # (uploaded on first use, outside any capture)
            s["bst"] = new((2, rows), i32, torch.zeros)
            s["bkept"] = new((2, rows), f64, torch.zeros)
            s["bsc"] = new((rows, k), f64)
        if mode.ctc:
            self.lens = mask.sum(dim=1).to(torch.int64).contiguous()
            self.flse = ctc_frame_lse(self.z, self.lens)
            s["ctc_state"] = ctc_prefix_state(b, n, k, lk, dev)
            s["cpsi"] = new((rows, k), f64)

    def clone_state(self, names=None) -> dict:
        """``state`` with the entries in ``names`` (default: all) copied, the rest shared."""
        return {key: _clone(v) if names is None or key in names else v
                for key, v in self.state.items()}

    def propose(self, t: int) -> None:
        """The decoder at position t and every live row's K best tokens, into ``cand``."""
        s, dec = self.state, self.dec
        self.hidden = dec.step(s["tok"], s["cache"], t, s["anc"][t & 1], s["skip"])
        seq_topk(self.hidden, dec.out.weight, dec.out.bias, self.mode.k, self.banned, s["skip"],
                 s["cand"])

    def score_ctc(self, t: int) -> None:
        """The candidates' CTC prefix scores, into ``cpsi``; ``ctc_state``'s table of t + 1."""
        s = self.state
        ctc_prefix_step(self.z, self.flse, self.lens, s["cand"][2], s["tok"], s["length"],
                        s["link"], s["skip"], s["ctc_state"][t & 1], s["ctc_state"][(t + 1) & 1],
                        s["cpsi"], self.ids["blank"], self.ids["eos"])

    def score_lm(self, t: int) -> None:
        """The candidates' LM scores, into ``lmsc``; ``lmctx``'s row of t + 1."""
        from .ngram import ngram_step

        s = self.state
        ngram_step(self.lm, s["cand"][2], s["tok"], s["length"], s["link"], s["skip"],
                   s["lmctx"][t & 1], s["lmctx"][(t + 1) & 1], s["lmsc"], self.n,
                   self.dec.out.weight.shape[0])

    def score_bias(self, t: int) -> None:
        """The candidates' bias values, into ``bsc``; ``bst`` / ``bkept``'s rows of t + 1."""
        from .bias import bias_step

        s = self.state
        bias_step(self.bias, s["cand"][2], s["tok"], s["length"], s["link"], s["skip"],
                  s["bst"][t & 1], s["bst"][(t + 1) & 1], s["bkept"][t & 1],
                  s["bkept"][(t + 1) & 1], s["bsc"], self.n, self.ids["eos"])

    def select(self, t: int, state: Optional[dict] = None) -> None:
        """The beam step: the N best keys of step t become the slots of step t + 1 (``state``:
        the buffers to run it on, default the search's own)."""
        s = self.state if state is None else state
        biased = self.bias is not None
        entry = BIASED_STEP if biased else self.mode.entry

        def ptrs(*names):
            return tuple(_lib.ptr(s.get(name)) for name in names)

        terms = ("att", "ctc", "lm", "bias") if biased else _STEP_TERMS[entry]
        args = tuple(x.data_ptr() for x in s["cand"])
        if terms:
            args += (_lib.ptr(s.get("cpsi")), self.w)
        if biased:   # the LM is optional: without one lmsc and lm are null and the weight is 0
            args += (_lib.ptr(s.get("lmsc")), self.lw if self.mode.lm else 0.0,
                     s["bsc"].data_ptr(), self.bw)
        elif "lm" in terms:
            args += (s["lmsc"].data_ptr(), self.lw)
        args += (self.b, self.n, self.mode.k, self.L, t, self.ids["eos"], self.ids["pad"],
                 s["norm"].data_ptr(), s["anc"][t & 1].data_ptr(),
                 s["anc"][(t + 1) & 1].data_ptr())
        args += ptrs("score", *terms, "length", "fin", "tok", "skip")
        if terms:
            args += ptrs("link")
        args += tuple(x.data_ptr() for x in s["trace"]) + (self.stream,)
        _lib.check(getattr(_lib.load(), entry)(*args), entry)

    def finish(self):
        """-> (hyp, hyp_len, n_hyp, score, info) of the slots as they stand."""
        if self.b == 0:
            return self.hyp, self.hyp_len, self.n_hyp, self.score_out, self.info
        s, info = self.state, self.info
        _lib.check(_lib.load().ob_attdec_finalize(
            s["trace"][0].data_ptr(), s["trace"][1].data_ptr(), s["score"].data_ptr(),
            s["length"].data_ptr(), s["fin"].data_ptr(), self.b, self.n, self.L, self.ids["eos"],
            self.hyp.data_ptr(), self.hyp_len.data_ptr(), self.n_hyp.data_ptr(),
            self.score_out.data_ptr(), self.finished.data_ptr(), self.stream),
            "ob_attdec_finalize")
        if self.info_keys:
            dead = s["fin"] == 2
            neg = torch.full_like(self.score_out, float("-inf"))
            for key in self.info_keys:
                if key == "att" and self.mode.entry == "ob_attdec_beam_step" and \
                        self.bias is None:
                    info["att"].copy_(self.score_out)       # S = A exactly
                else:
                    info[key].copy_(torch.where(dead, neg, s[key]))
        return self.hyp, self.hyp_len, self.n_hyp, self.score_out, info

    def run(self):
        if self.b > 0:
            for t in range(self.L):
                self.propose(t)
                if self.mode.ctc:
                    self.score_ctc(t)
                if self.mode.lm:
                    self.score_lm(t)
                if self.bias is not None:
                    self.score_bias(t)
                self.select(t)
        return self.finish()
