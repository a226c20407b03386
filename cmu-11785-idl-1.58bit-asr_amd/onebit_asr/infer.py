"""Inference path (BASELINE configs[4]): packed-ternary weights, optional int8 activations,
batched greedy CTC decode -- the encoder + CTC head forward of the reference's eval loop
(eval.py:91-124: ``model(batch, precision)``, valid lengths from the mask) followed by
metrics.py:51-60's greedy decode, for a whole padded batch at once.

* weights: each QuantizedLinear's 2-bit codes are packed once and cached (they are only
  repacked when a weight or alpha changes), so a forward streams 2-bit codes, never W;
* activations: ``act_quant="absmax_int8"`` runs the BitLinear GEMMs on the int8 matrix
  cores (the north-star mode, csrc/tgemm_i8.hip); ``None`` keeps the reference's fp32;
* decode: ``ob_ctc_greedy_decode`` (csrc/decode.hip), argmax + collapse on the device; with
  ``decoder="beam"`` the reference's prefix beam search (metrics.py:74-145) instead,
  ``ob_ctc_beam_search`` (csrc/beam.hip); with ``decoder="rescore"`` two-pass decoding: the
  CTC n-best (``ob_ctc_beam_search_nbest``) is scored by the attention decoder under teacher
  forcing against the shared encoder memory, the output layer and its log-softmax run fused
  (``ob_seq_logprob``, csrc/rescore.hip), and the best ``att + ctc_weight * ctc`` wins; with
  ``decoder="attention"`` the attention decoder writes the transcript itself: KV-cached beam
  search at a static length (``attention_beam_search``, onebit_asr/attdec.py, csrc/attdec.hip);
  with an n-gram LM and ``lm_fusion="first_pass"`` the LM runs inside the prefix beam search
  (``ob_ctc_beam_search_lm``) instead of re-ranking its n-best;
* ``GraphedInference`` captures forward + decode as one HIP graph for a fixed padded shape;
* ``frontend=FrontEnd(...)`` (onebit_asr/frontend.py) puts the feature kernel ahead of the
  encoder: the batch then carries ``wave`` / ``wave_lens`` in place of ``feats`` / ``feat_lens``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .attdec import MAX_BEAM, SPECIAL  # the token ids; 32 is ob_ctc_beam_search's beam limit too
from .quant import set_act_quant

__all__ = ["ctc_greedy_decode_batch", "ctc_greedy_decode", "ctc_beam_search_batch_device",
           "ctc_beam_search_nbest_device", "ctc_beam_search_lm_device",
           "ctc_beam_search_bias_device", "seq_logprob",
           "attention_rescore", "ctc_lm_rescore", "GraphedInference", "encode_and_decode"]

DECODERS = ("greedy", "beam", "rescore", "attention")


def ctc_greedy_decode_batch(logits: torch.Tensor, lens: torch.Tensor, blank_id: int = 3
                            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits [B, T, V] fp32 (device), lens [B] valid frames -> (tokens int32 [B, T], padded
    with -1; counts int32 [B]). No host synchronisation."""
    if not logits.is_cuda:
        raise RuntimeError("ctc_greedy_decode_batch runs on the HIP library (no CPU fallback)")
    b, t, v = logits.shape
    x = logits.contiguous().float()
    ln = lens.to(device=x.device, dtype=torch.int64).contiguous()
    ids = torch.empty((b, t), dtype=torch.int32, device=x.device)
    out = torch.empty((b, t), dtype=torch.int32, device=x.device)
    cnt = torch.empty((b,), dtype=torch.int32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.ob_ctc_greedy_decode(x.data_ptr(), ln.data_ptr(), b, t, v, blank_id,
                                        ids.data_ptr(), out.data_ptr(), cnt.data_ptr(),
                                        _lib.stream_of(x)), "ob_ctc_greedy_decode")
    return out, cnt


def ctc_greedy_decode(logits: torch.Tensor, blank_id: int = 3) -> List[int]:
    """metrics.py:51-60 signature: one utterance's logits [T, V] -> token list."""
    t = logits.size(0)
    out, cnt = ctc_greedy_decode_batch(logits.unsqueeze(0),
                                       torch.tensor([t], device=logits.device), blank_id)
    n = int(cnt.item())
    return out[0, :n].tolist()


MAX_TOP_K = 64  # with MAX_BEAM, ob_ctc_beam_search's argument limits (include/onebit_hip.h)


def _beam_args(logits, beam_size, blank_id, top_k_per_t):
    b, t, v = logits.shape
    if not 1 <= beam_size <= MAX_BEAM:
        raise ValueError(f"beam_size must be in 1..{MAX_BEAM}, got {beam_size}")
    if top_k_per_t is None:
        if v > MAX_TOP_K:
            raise ValueError(f"top_k_per_t=None (all tokens) needs V <= {MAX_TOP_K}, got V = {v}")
        top_k = v
    elif not 1 <= top_k_per_t <= MAX_TOP_K:
        raise ValueError(f"top_k_per_t must be in 1..{MAX_TOP_K} or None, got {top_k_per_t}")
    else:
        top_k = top_k_per_t
    if not 0 <= blank_id < v:
        raise ValueError(f"blank_id {blank_id} outside the vocabulary of {v}")
    return top_k


def _ctc_beam(fn, logits, lens, beam_size, blank_id, top_k_per_t, nbest=None, fused=None):
    """The one call path of the three searches, for the public function ``fn``. ``nbest=None``:
    the 1-best form (``ob_ctc_beam_search``), else ``ob_ctc_beam_search_nbest``; ``fused`` =
    (lm, lm_weight, ins_bonus): ``ob_ctc_beam_search_lm``. Returns (hyp, hyp_len, n_hyp or None,
    the score tensors: one, or ctc / lm / total)."""
    if not logits.is_cuda:
        raise RuntimeError(f"{fn} runs on the HIP library (no CPU fallback)")
    b, t, v = logits.shape
    top_k = _beam_args(logits, beam_size, blank_id, top_k_per_t)
    if nbest is not None and not 1 <= nbest <= beam_size:
        raise ValueError(f"nbest must be in 1..beam_size ({beam_size}), got {nbest}")
    lib = _lib.load()
    if fused is None:
        need = lib.ob_ctc_beam_search_workspace(b, t, v, beam_size, top_k)
        if b > 0 and need == 0:
            raise ValueError(f"ctc beam search: shape B={b} T={t} V={v} is not supported")
    else:
        lm, lm_weight, ins_bonus = fused[0], float(fused[1]), float(fused[2])
        if not 0 <= lm_weight < float("inf"):
            raise ValueError(f"lm_weight must be >= 0 and finite, got {lm_weight}")
        if not abs(ins_bonus) < float("inf"):
            raise ValueError(f"ins_bonus must be finite, got {ins_bonus}")
        if lm is None:
            raise ValueError(f"{fn} needs an NGramLM")
        if (SPECIAL["bos"], SPECIAL["eos"]) != (lm.bos, lm.eos):
            raise ValueError(f"the LM's bos / eos are {lm.bos} / {lm.eos}, the decoder's "
                             f"{SPECIAL['bos']} / {SPECIAL['eos']}")
        need = lib.ob_ctc_beam_search_lm_workspace(b, t, v, beam_size, top_k, lm.order)
        if need == 0 and (b > 0 or lib.ob_ctc_beam_search_lm_workspace(1, t, v, beam_size, top_k,
                                                                       lm.order) == 0):
            raise ValueError(f"ctc beam search with an LM: shape B={b} T={t} V={v} "
                             f"order={lm.order} is not supported (order <= 4, V <= 65535)")
    x = logits.contiguous().float()
    ln = lens.to(device=x.device, dtype=torch.int64).contiguous()
    rows = (b,) if nbest is None else (b, nbest)
    hyp = torch.empty(rows + (t,), dtype=torch.int32, device=x.device)
    hyp_len = torch.empty(rows, dtype=torch.int32, device=x.device)
    n_hyp = None if nbest is None else torch.empty((b,), dtype=torch.int32, device=x.device)
    scores = [torch.empty(rows, dtype=torch.float64, device=x.device)
              for _ in range(1 if fused is None else 3)]
    form = () if nbest is None else (nbest,)
    if fused is not None:
        table, slots, max_probe, order, _, unk = lm._args(x.device, v)
        form += (table, slots, max_probe, order, unk, lm.bos, lm.eos, lm_weight, ins_bonus)
    ws = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=x.device)
    entry = "ob_ctc_beam_search" + ("" if nbest is None else "_nbest" if fused is None else "_lm")
    outs = [o.data_ptr() for o in (hyp, hyp_len, n_hyp, *scores) if o is not None]
    _lib.check(getattr(lib, entry)(x.data_ptr(), ln.data_ptr(), b, t, v, blank_id, beam_size,
                                   top_k, *form, ws.data_ptr(), ws.numel() * 8, *outs,
                                   _lib.stream_of(x)), entry)
    return hyp, hyp_len, n_hyp, scores


def ctc_beam_search_batch_device(logits: torch.Tensor, lens: torch.Tensor, beam_size: int = 10,
                                 blank_id: int = 3, top_k_per_t: Optional[int] = 20
                                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CTC prefix beam search of metrics.py:74-145 for a whole padded batch on the device.
    logits [B, T, V] fp32 (device), lens [B] valid frames -> (tokens int32 [B, T], padded with
    -1; counts int32 [B]; scores float64 [B], the log-probability of each returned prefix).
    ``top_k_per_t=None`` means every token and needs V <= 64. No host synchronisation; the
    workspace comes from the caching allocator."""
    out, cnt, _, (score,) = _ctc_beam("ctc_beam_search_batch_device", logits, lens, beam_size,
                                      blank_id, top_k_per_t)
    return out, cnt, score


def ctc_beam_search_nbest_device(logits: torch.Tensor, lens: torch.Tensor, beam_size: int = 10,
                                 nbest: Optional[int] = None, blank_id: int = 3,
                                 top_k_per_t: Optional[int] = 20):
    """The search of ``ctc_beam_search_batch_device`` returning the final beam's first
    ``nbest`` entries (default: all ``beam_size``), best first: (hyp int32 [B, nbest, T] padded
    with -1, hyp_len int32 [B, nbest], n_hyp int32 [B] live entries, scores float64 [B, nbest],
    -inf for absent entries). Entry 0 is the 1-best call's result bit for bit. No host
    synchronisation."""
    hyp, hyp_len, n_hyp, (score,) = _ctc_beam(
        "ctc_beam_search_nbest_device", logits, lens, beam_size, blank_id, top_k_per_t,
        nbest=beam_size if nbest is None else nbest)
    return hyp, hyp_len, n_hyp, score


def ctc_beam_search_lm_device(logits: torch.Tensor, lens: torch.Tensor, lm, lm_weight: float,
                              ins_bonus: float = 0.0, beam_size: int = 10,
                              nbest: Optional[int] = None, blank_id: int = 3,
                              top_k_per_t: Optional[int] = 20):
    """The search of ``ctc_beam_search_nbest_device`` with the n-gram LM ``lm`` (an
    ``ngram.NGramLM``) inside it (``ob_ctc_beam_search_lm``): a frame keeps the ``beam_size``
    prefixes with the largest ``(ctc + lm_weight * lm(y)) + ins_bonus * len(y)``, and the final beam
    is ordered by that total with the closing eos scored. Returns (hyp int32 [B, nbest, T] padded
    with -1, hyp_len int32 [B, nbest], n_hyp int32 [B], info = {ctc, lm, total}, float64
    [B, nbest], -inf for absent entries); ``lm`` includes the eos. ``lm_weight`` >= 0;
    ``ins_bonus`` is the insertion bonus per token, any finite value. The table is uploaded on the
    first call for a device. No host synchronisation."""
    hyp, hyp_len, n_hyp, (ctc, lms, total) = _ctc_beam(
        "ctc_beam_search_lm_device", logits, lens, beam_size, blank_id, top_k_per_t,
        nbest=beam_size if nbest is None else nbest, fused=(lm, lm_weight, ins_bonus))
    return hyp, hyp_len, n_hyp, {"ctc": ctc, "lm": lms, "total": total}


def _check_bias_weight(bias, bias_weight: float) -> float:
    bias_weight = float(bias_weight)
    if not 0 <= bias_weight < float("inf"):
        raise ValueError(f"bias_weight must be >= 0 and finite, got {bias_weight}")
    if bias_weight != 0 and bias is None:
        raise ValueError("bias_weight is set but bias is None")
    return bias_weight


def ctc_beam_search_bias_device(logits: torch.Tensor, lens: torch.Tensor, bias, bias_weight: float,
                                lm=None, lm_weight: float = 0.0, ins_bonus: float = 0.0,
                                beam_size: int = 10, nbest: Optional[int] = None,
                                blank_id: int = 3, top_k_per_t: Optional[int] = 20):
    """The search of ``ctc_beam_search_lm_device`` with the phrase list ``bias`` (a
    ``bias.ContextBias``) inside it (``ob_ctc_beam_search_bias``): a frame keeps the ``beam_size``
    prefixes with the largest ``((ctc + lm_weight * lm(y)) + ins_bonus * len(y)) + bias_weight *
    bias(y)``, bias(y) the running value with partial matches counted, and the final beam is
    ordered by the total with the closing eos scored and ``bias_fin(y)``, which takes an unfinished
    match back. ``lm=None`` is the search without an LM (``lm_weight`` must then be 0; ``lm`` is 0
    for present entries). Returns (hyp int32 [B, nbest, T] padded with -1, hyp_len int32
    [B, nbest], n_hyp int32 [B], info = {ctc, lm, bias, total}, float64 [B, nbest], -inf for absent
    entries). With ``bias_weight == 0`` the result is ``ctc_beam_search_lm_device``'s bit for bit,
    and without an LM and ``ins_bonus`` also ``ctc_beam_search_nbest_device``'s. The tables are
    uploaded on the first call for a device. No host synchronisation."""
    fn = "ctc_beam_search_bias_device"
    if not logits.is_cuda:
        raise RuntimeError(f"{fn} runs on the HIP library (no CPU fallback)")
    if bias is None:
        raise ValueError(f"{fn} needs a ContextBias")
    bias_weight = _check_bias_weight(bias, bias_weight)
    lm_weight, ins_bonus = float(lm_weight), float(ins_bonus)
    if not 0 <= lm_weight < float("inf"):
        raise ValueError(f"lm_weight must be >= 0 and finite, got {lm_weight}")
    if not abs(ins_bonus) < float("inf"):
        raise ValueError(f"ins_bonus must be finite, got {ins_bonus}")
    if lm is None and lm_weight != 0:
        raise ValueError("lm_weight is set but lm is None")
    if lm is not None and (SPECIAL["bos"], SPECIAL["eos"]) != (lm.bos, lm.eos):
        raise ValueError(f"the LM's bos / eos are {lm.bos} / {lm.eos}, the decoder's "
                         f"{SPECIAL['bos']} / {SPECIAL['eos']}")
    b, t, v = logits.shape
    top_k = _beam_args(logits, beam_size, blank_id, top_k_per_t)
    nbest = beam_size if nbest is None else nbest
    if not 1 <= nbest <= beam_size:
        raise ValueError(f"nbest must be in 1..beam_size ({beam_size}), got {nbest}")
    lib = _lib.load()
    order = 0 if lm is None else lm.order
    need = lib.ob_ctc_beam_search_bias_workspace(b, t, v, beam_size, top_k, order, bias.n_nodes)
    if need == 0 and (b > 0 or lib.ob_ctc_beam_search_bias_workspace(
            1, t, v, beam_size, top_k, order, bias.n_nodes) == 0):
        raise ValueError(f"ctc beam search with a bias: shape B={b} T={t} V={v} order={order} is "
                         "not supported (order <= 4, V <= 65535)")
    x = logits.contiguous().float()
    ln = lens.to(device=x.device, dtype=torch.int64).contiguous()
    hyp = torch.empty((b, nbest, t), dtype=torch.int32, device=x.device)
    hyp_len = torch.empty((b, nbest), dtype=torch.int32, device=x.device)
    n_hyp = torch.empty((b,), dtype=torch.int32, device=x.device)
    ctc, lms, bs, total = (torch.empty((b, nbest), dtype=torch.float64, device=x.device)
                           for _ in range(4))
    if lm is None:
        lm_args = (None, 0, 0, 0, 0.0, SPECIAL["bos"], SPECIAL["eos"], 0.0, ins_bonus)
    else:
        table, slots, max_probe, _, _, unk = lm._args(x.device, v)
        lm_args = (table, slots, max_probe, order, unk, lm.bos, lm.eos, lm_weight, ins_bonus)
    ws = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=x.device)
    _lib.check(lib.ob_ctc_beam_search_bias(
        x.data_ptr(), ln.data_ptr(), b, t, v, blank_id, beam_size, top_k, nbest, *lm_args,
        *bias._args(x.device), bias_weight, ws.data_ptr(), ws.numel() * 8, hyp.data_ptr(),
        hyp_len.data_ptr(), n_hyp.data_ptr(), ctc.data_ptr(), lms.data_ptr(), bs.data_ptr(),
        total.data_ptr(), _lib.stream_of(x)), "ob_ctc_beam_search_bias")
    return hyp, hyp_len, n_hyp, {"ctc": ctc, "lm": lms, "bias": bs, "total": total}


def seq_logprob(hidden: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                target: torch.Tensor) -> torch.Tensor:
    """``log_softmax(hidden @ weight.T + bias)[r, target[r]]`` per row without the [R, V] logits
    (``ob_seq_logprob``): hidden [R, d] fp32, weight [V, d], bias [V] or None, target int32 [R]
    (-1 = skip the row, result 0) -> float32 [R]. d % 16 == 0, d <= 256."""
    if not hidden.is_cuda:
        raise RuntimeError("seq_logprob runs on the HIP library (no CPU fallback)")
    h = hidden.contiguous().float()
    w = weight.detach().contiguous().float()
    bs = bias.detach().contiguous().float() if bias is not None else None
    tg = target.to(device=h.device, dtype=torch.int32).contiguous()
    r, d = h.shape
    v = w.shape[0]
    if w.shape[1] != d or tg.shape != (r,) or (bs is not None and bs.shape != (v,)):
        raise ValueError(f"seq_logprob: hidden {tuple(h.shape)}, weight {tuple(w.shape)}, target "
                         f"{tuple(tg.shape)} do not match")
    lib = _lib.load()
    need = lib.ob_seq_logprob_workspace(r, d, v)
    if need == 0 and (r > 0 or lib.ob_seq_logprob_workspace(1, d, v) == 0):
        raise ValueError(f"seq_logprob: shape R={r} d={d} V={v} is not supported "
                         "(d % 16 == 0, 16 <= d <= 256)")
    ws = torch.empty((max(need, 8) // 8,), dtype=torch.int64, device=h.device)
    lp = torch.empty((r,), dtype=torch.float32, device=h.device)
    _lib.check(lib.ob_seq_logprob(h.data_ptr(), r, d, w.data_ptr(), _lib.ptr(bs), v,
                                  tg.data_ptr(), ws.data_ptr(), ws.numel() * 8, lp.data_ptr(),
                                  _lib.stream_of(h)), "ob_seq_logprob")
    return lp


@torch.no_grad()
def attention_rescore(model, enc: torch.Tensor, mask: torch.Tensor, hyp: torch.Tensor,
                      hyp_len: torch.Tensor, n_hyp: torch.Tensor, ctc_scores: torch.Tensor,
                      ctc_weight: float = 0.5, max_len: Optional[int] = None,
                      special: Optional[Dict[str, int]] = None, lm=None, lm_weight: float = 0.0):
    """Second pass of two-pass decoding: score the n-best ``hyp`` [B, N, T] (the outputs of
    ``ctc_beam_search_nbest_device``) with ``model.decoder`` under teacher forcing on the
    encoder output ``enc`` [B, T', d] / ``mask`` [B, T'], and return the hypothesis with the
    largest ``att + ctc_weight * ctc_score`` per utterance (ties: the better CTC rank).

    Returns (out int32 [B, T] padded with -1, cnt int32 [B], info) with info = {best_k int32
    [B], att float64 [B, N], total float64 [B, N], rescored bool [B]}. Hypotheses are scored at
    the static length ``max_len``; an utterance with a live hypothesis longer than that is not
    rescored: it returns its CTC best and ``rescored`` False. ``max_len=None`` reads the
    longest hypothesis length back from the device, which SYNCHRONISES with the host -- eager
    mode only; a captured graph needs an explicit ``max_len``. ``special``: token ids, default
    ``{"pad": 0, "bos": 1, "eos": 2, "blank": 3}``.

    ``lm`` (an ``ngram.NGramLM``) with ``lm_weight`` != 0 adds the LM score of every hypothesis
    (``ob_ngram_seq_logprob``, eos included): total = (att + ctc_weight * ctc) + lm_weight * lm
    (``ob_rescore_select_lm``) and info also holds ``lm`` float64 [B, N] (-inf for absent
    entries). ``lm=None`` or ``lm_weight == 0`` is the pass without an LM, unchanged."""
    if not enc.is_cuda:
        raise RuntimeError("attention_rescore runs on the HIP library (no CPU fallback)")
    ids = dict(SPECIAL, **(special or {}))
    b, n, t = hyp.shape
    dev = enc.device
    hyp = hyp.to(device=dev, dtype=torch.int32).contiguous()
    hyp_len = hyp_len.to(device=dev, dtype=torch.int32).contiguous()
    n_hyp = n_hyp.to(device=dev, dtype=torch.int32).contiguous()
    ctc = ctc_scores.to(device=dev, dtype=torch.float64).contiguous()
    if max_len is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("attention_rescore: a captured graph needs an explicit max_len")
        max_len = int(hyp_len.max().item()) if b > 0 else 0  # host synchronisation
    lc = int(max_len)
    if lc < 0:
        raise ValueError(f"max_len must be >= 0, got {max_len}")
    rows = b * n
    tgt_inp = torch.empty((rows, lc + 1), dtype=torch.int64, device=dev)
    target = torch.empty((rows, lc + 1), dtype=torch.int32, device=dev)
    tgt_pad = torch.empty((rows, lc + 1), dtype=torch.uint8, device=dev)
    ok = torch.empty((b,), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().ob_rescore_prepare(
        hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(), b, n, t, lc, ids["bos"], ids["eos"],
        ids["pad"], tgt_inp.data_ptr(), target.data_ptr(), tgt_pad.data_ptr(), ok.data_ptr(),
        _lib.stream_of(enc)), "ob_rescore_prepare")
    if b > 0:
        dec = model.decoder
        h = dec.hidden(tgt_inp, enc, mask, tgt_pad.view(torch.bool), mem_group=n)
        lp = seq_logprob(h.reshape(rows * (lc + 1), h.shape[-1]), dec.out.weight, dec.out.bias,
                         target.reshape(-1))
    else:
        lp = torch.empty((0,), dtype=torch.float32, device=dev)
    lms = None
    if lm is not None and lm_weight != 0:
        lms = _nbest_lm(lm, hyp, hyp_len, n_hyp, model.decoder.out.weight.shape[0], ids)
    return _rescore_pick(hyp, hyp_len, n_hyp, ctc, lms, lp, ok, lc, ctc_weight, lm_weight)


def _rescore_pick(hyp, hyp_len, n_hyp, ctc, lms, lp, ok, lc, ctc_weight, lm_weight):
    """The pick of the best total per utterance: ``ob_rescore_select``, with ``lms`` (float64
    [B, N]) ``ob_rescore_select_lm``; ``lp`` / ``ok`` None: no attention pass (needs ``lms``).
    Returns (out, cnt, info); info holds ``att`` / ``rescored`` only with an attention pass."""
    b, n, t = hyp.shape
    dev = hyp.device
    out = torch.empty((b, t), dtype=torch.int32, device=dev)
    cnt = torch.empty((b,), dtype=torch.int32, device=dev)
    best_k = torch.empty((b,), dtype=torch.int32, device=dev)
    total = torch.empty((b, n), dtype=torch.float64, device=dev)
    rescored = torch.empty((b,), dtype=torch.uint8, device=dev)
    att = None if lp is None else torch.empty((b, n), dtype=torch.float64, device=dev)
    entry = "ob_rescore_select" if lms is None else "ob_rescore_select_lm"
    lm_ptr, lm_w = ((), ()) if lms is None else ((lms.data_ptr(),), (float(lm_weight),))
    _lib.check(getattr(_lib.load(), entry)(
        _lib.ptr(lp), hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(), ctc.data_ptr(),
        *lm_ptr, _lib.ptr(ok), b, n, t, lc, float(ctc_weight), *lm_w, out.data_ptr(),
        cnt.data_ptr(), best_k.data_ptr(), _lib.ptr(att), total.data_ptr(), rescored.data_ptr(),
        _lib.stream_of(hyp)), entry)
    info = {"best_k": best_k, "total": total}
    if lp is not None:
        info.update(att=att, rescored=rescored.view(torch.bool))
    if lms is not None:
        info["lm"] = lms
    return out, cnt, info


def _nbest_lm(lm, hyp, hyp_len, n_hyp, vocab_size, ids) -> torch.Tensor:
    """The LM score of every n-best entry, float64 [B, N]; absent entries (k >= n_hyp[b]): -inf."""
    from .ngram import ngram_seq_logprob

    if (ids["bos"], ids["eos"]) != (lm.bos, lm.eos):
        raise ValueError(f"the LM's bos / eos are {lm.bos} / {lm.eos}, the decoder's "
                         f"{ids['bos']} / {ids['eos']}")
    n = hyp.shape[1]
    live = torch.arange(n, device=hyp.device)[None, :] < n_hyp[:, None]
    return ngram_seq_logprob(lm, hyp, torch.where(live, hyp_len, torch.full_like(hyp_len, -1)),
                             vocab_size)


def ctc_lm_rescore(hyp: torch.Tensor, hyp_len: torch.Tensor, n_hyp: torch.Tensor,
                   ctc_scores: torch.Tensor, lm, lm_weight: float, vocab_size: int,
                   special: Optional[Dict[str, int]] = None):
    """The CTC n-best (``ctc_beam_search_nbest_device``'s outputs) picked by ``ctc + lm_weight *
    lm`` (``ob_ngram_seq_logprob`` + ``ob_rescore_select_lm`` without an attention pass; ties to
    the better CTC rank). Returns (out int32 [B, T] padded with -1, cnt int32 [B], info = {best_k
    int32 [B], lm float64 [B, N], total float64 [B, N]}). No host synchronisation."""
    if not hyp.is_cuda:
        raise RuntimeError("ctc_lm_rescore runs on the HIP library (no CPU fallback)")
    ids = dict(SPECIAL, **(special or {}))
    b, n, t = hyp.shape
    dev = hyp.device
    hyp = hyp.to(torch.int32).contiguous()
    hyp_len = hyp_len.to(device=dev, dtype=torch.int32).contiguous()
    n_hyp = n_hyp.to(device=dev, dtype=torch.int32).contiguous()
    ctc = ctc_scores.to(device=dev, dtype=torch.float64).contiguous()
    lms = _nbest_lm(lm, hyp, hyp_len, n_hyp, vocab_size, ids)
    return _rescore_pick(hyp, hyp_len, n_hyp, ctc, lms, None, None, 0, 1.0, lm_weight)


def _check_lm(decoder: str, lm, lm_weight: float) -> bool:
    """-> whether the LM takes part."""
    if lm_weight < 0 or lm_weight != lm_weight:
        raise ValueError(f"lm_weight must be >= 0, got {lm_weight}")
    if decoder == "greedy" and lm_weight != 0:
        raise ValueError("lm_weight needs decoder 'beam', 'rescore' or 'attention': greedy "
                         "decoding has no hypotheses to weigh")
    if lm_weight != 0 and lm is None:
        raise ValueError("lm_weight is set but lm is None")
    return lm is not None and lm_weight != 0


LM_FUSIONS = ("rescore", "first_pass")


def _check_fusion(decoder: str, use_lm: bool, lm_fusion: str, ins_bonus: float) -> bool:
    """-> whether the LM runs inside the CTC prefix beam search."""
    if lm_fusion not in LM_FUSIONS:
        raise ValueError(f"lm_fusion must be 'rescore' or 'first_pass', got {lm_fusion!r}")
    if not abs(float(ins_bonus)) < float("inf"):
        raise ValueError(f"ins_bonus must be finite, got {ins_bonus}")
    if lm_fusion != "first_pass":
        if ins_bonus != 0:
            raise ValueError("ins_bonus needs lm_fusion='first_pass': re-ranking has no use for it")
        return False
    if decoder != "beam":
        raise ValueError("lm_fusion='first_pass' needs decoder='beam' (the other decoders already "
                         f"run with the LM inside the search), got decoder={decoder!r}")
    if not use_lm:
        raise ValueError("lm_fusion='first_pass' needs an lm and lm_weight > 0")
    return True


def _check_bias(decoder: str, bias, bias_weight: float, use_lm: bool, first_pass: bool) -> bool:
    """-> whether the phrase list takes part."""
    bias_weight = _check_bias_weight(bias, bias_weight)
    if bias is None or bias_weight == 0:
        return False
    if decoder in ("greedy", "rescore"):
        raise ValueError("bias_weight needs decoder 'beam' or 'attention': greedy decoding has no "
                         "hypotheses to weigh and the rescoring total has no bias term")
    if decoder == "beam" and use_lm and not first_pass:
        raise ValueError("decoder='beam' with a bias and an lm needs lm_fusion='first_pass' (the "
                         "biased search carries the LM inside it)")
    return True


def _check_timestamps(timestamps) -> None:
    # the keyword sits ahead of joint_ctc_weight / ctc_cand: a weight passed by position must not
    # be taken for it
    if not isinstance(timestamps, bool):
        raise TypeError(f"timestamps must be a bool, got {timestamps!r}")


def _check_mbr(decoder: str, mbr_scale: Optional[float]) -> Optional[float]:
    if mbr_scale is None:
        return None
    from .edit import check_mbr_scale

    if decoder == "greedy":
        raise ValueError("mbr_scale needs decoder 'beam', 'rescore' or 'attention': greedy "
                         "decoding has no n-best to choose from")
    return check_mbr_scale(mbr_scale)


def _check_joint(decoder: str, joint_ctc_weight: float) -> None:
    if not 0.0 <= float(joint_ctc_weight) <= 1.0:
        raise ValueError(f"joint_ctc_weight must be in [0, 1], got {joint_ctc_weight}")
    if joint_ctc_weight != 0 and decoder != "attention":
        raise ValueError("joint_ctc_weight needs decoder='attention' (the joint CTC/attention "
                         f"search), got decoder={decoder!r}")


@torch.no_grad()
def encode_and_decode(model, batch: Dict[str, torch.Tensor], precision: int = 2,
                      blank_id: int = 3, decoder: str = "greedy", beam_size: int = 10,
                      frontend=None, ctc_weight: float = 0.5, max_len: Optional[int] = None,
                      info: Optional[dict] = None, length_penalty: float = 0.0,
                      timestamps: bool = False, *, mbr_scale: Optional[float] = None, bias=None,
                      bias_weight: float = 0.0, lm=None, lm_weight: float = 0.0,
                      lm_fusion: str = "rescore", ins_bonus: float = 0.0,
                      joint_ctc_weight: float = 0.0, ctc_cand: Optional[int] = None):
    """Encoder + CTC head + decode of one padded batch (eval.py:118-124 for one precision).
    ``decoder="greedy"`` (the default) or ``"beam"``, the reference's beam search with its
    eval settings (beam_size, the 20 best tokens per frame). With ``frontend`` (a ``FrontEnd``)
    the batch holds ``wave`` [B, n_max] and ``wave_lens`` [B] and the features are computed
    here, on the same stream; its other entries (``tokens``...) pass through.
    ``decoder="rescore"``: the beam search's n-best (all ``beam_size`` entries) rescored by the
    attention decoder (``attention_rescore`` with ``ctc_weight`` / ``max_len``; ``max_len=None``
    synchronises with the host); a dict passed as ``info`` receives its best_k / att / total /
    rescored and the n-best itself (hyp, hyp_len, n_hyp, ctc_scores, enc, mask).
    ``decoder="attention"``: beam search with the attention decoder (``attention_beam_search``
    with ``beam_size`` / ``max_len``, default 64, / ``length_penalty``); tokens are then
    [B, max_len], the best hypothesis padded with -1, and ``info`` receives the n-best (hyp,
    hyp_len, n_hyp, score), finished, the trace, enc and mask. With ``joint_ctc_weight`` w > 0
    the search is the one-pass joint CTC/attention decode (``joint_beam_search`` on the logits of
    this forward, ``ctc_cand`` attention candidates per slot): score is then
    (1 - w) * att + w * ctc and ``info`` also receives ``att`` / ``ctc``; w == 0 is the
    attention-only search, unchanged.
    ``timestamps=True`` (a bool; pass it by keyword): after any decoder the returned (tokens,
    counts) are force-aligned against this forward's logits (``align.ctc_forced_align``, the first
    511 tokens at most) and ``info`` receives ``span`` int32 [B, S, 2], ``tok_score`` float64
    [B, S], ``align_score`` float64 [B] and ``frame_path`` int32 [B, T']. The output of "greedy"
    and "beam" always has a CTC alignment; that of "rescore", "attention" and the joint search may
    not (more tokens than frames, a repeat without a frame for its blank): ``align_score`` is
    then -inf and the utterance's spans and frame_path are -1. ``False`` is the path without it.
    ``lm`` (an ``ngram.NGramLM``) with ``lm_weight`` > 0 is n-gram shallow fusion (keyword only,
    as everything after ``timestamps``: tests/test_joint_cpu.py pins ``joint_ctc_weight`` /
    ``ctc_cand`` as the last parameters, so the marker sits ahead of all four):
    "attention" runs ``joint_beam_search`` with the LM (``joint_ctc_weight`` 0: attention + LM) and
    ``info`` also receives ``att`` / ``ctc`` / ``lm``; "rescore" adds ``lm_weight * lm`` to every
    total (``info["lm"]``); "beam" takes the CTC n-best (``beam_size`` entries) and returns the
    entry with the largest ``ctc + lm_weight * lm``, the attention decoder does not run, and
    ``info`` receives hyp, hyp_len, n_hyp, ctc_scores, lm, total and best_k; "greedy" with
    ``lm_weight != 0`` is a ValueError. ``lm=None`` or ``lm_weight == 0`` changes nothing.
    ``lm_fusion="first_pass"`` (keyword only; "beam" with an LM and ``lm_weight`` > 0, anything
    else is a ValueError) puts the LM inside the CTC prefix beam search instead of re-ranking its
    n-best (``ctc_beam_search_lm_device`` with ``nbest = beam_size`` and the insertion bonus
    ``ins_bonus`` per token): the result is entry 0 and ``info`` receives hyp, hyp_len, n_hyp,
    ctc_scores, lm, total and best_k (zeros). The default ``"rescore"`` is every decoder's
    behaviour described above.
    ``mbr_scale`` (keyword only; ``None`` is every path above, untouched): a float >= 0 replaces
    the "largest total" pick by minimum-Bayes-risk selection (``edit.mbr_select`` with that scale)
    over the n-best the decoder produced and the totals it ranks them by: "beam" then takes the
    n-best search (``beam_size`` entries) and its CTC scores; "beam" with an LM the
    ``ctc + lm_weight * lm`` totals, in either fusion mode; "rescore" its ``total``; "attention"
    and the joint search ``score``. ``info`` receives the decoder's entries as above and
    ``mbr_risk`` / ``mbr_post`` float64 [B, N], ``map_k`` (the entry returned without MBR) and
    ``best_k`` (the MBR pick). "greedy" with ``mbr_scale`` is a ValueError, as is a negative or
    non-finite value.
    ``bias`` (a ``bias.ContextBias``) with ``bias_weight`` > 0 (keyword only) is phrase-list
    contextual biasing: "beam" runs ``ctc_beam_search_bias_device`` (with an LM it needs
    ``lm_fusion="first_pass"``, else a ValueError) and ``info`` receives the first-pass entries plus
    ``bias``; "attention" runs ``joint_beam_search`` with the bias, whatever ``joint_ctc_weight``
    and ``lm`` are, and ``info`` also receives ``bias``. "greedy" and "rescore" with
    ``bias_weight != 0`` are ValueErrors, as are a negative or non-finite weight and a weight
    without a bias object. ``bias=None`` or ``bias_weight == 0`` changes nothing; ``mbr_scale`` and
    ``timestamps`` work on the result as above.
    Returns (tokens, counts, logits)."""
    if decoder not in DECODERS:
        raise ValueError("decoder must be 'greedy', 'beam', 'rescore' or 'attention', got "
                         f"{decoder!r}")
    _check_joint(decoder, joint_ctc_weight)
    _check_timestamps(timestamps)
    use_lm = _check_lm(decoder, lm, lm_weight)
    first_pass = _check_fusion(decoder, use_lm, lm_fusion, ins_bonus)
    use_bias = _check_bias(decoder, bias, bias_weight, use_lm, first_pass)
    mbr_scale = _check_mbr(decoder, mbr_scale)
    if mbr_scale is not None and info is None:
        info = {}
    if frontend is not None:
        rest = {k: v for k, v in batch.items() if k not in ("wave", "wave_lens")}
        batch = {**rest, **frontend(batch["wave"], batch["wave_lens"])}
    enc, mask, logits = model(batch, precision=precision)
    lens = mask.sum(dim=1)
    if decoder == "attention":
        from .attdec import attention_beam_search, joint_beam_search

        if use_bias:
            hyp, hyp_len, n_hyp, scores, res = joint_beam_search(
                model, enc, mask, logits, beam_size, 64 if max_len is None else max_len,
                joint_ctc_weight, ctc_cand, length_penalty, {"blank": blank_id}, lm, lm_weight,
                bias, float(bias_weight))
        elif use_lm or joint_ctc_weight > 0:
            hyp, hyp_len, n_hyp, scores, res = joint_beam_search(
                model, enc, mask, logits, beam_size, 64 if max_len is None else max_len,
                joint_ctc_weight, ctc_cand, length_penalty, {"blank": blank_id}, lm, lm_weight)
        else:
            hyp, hyp_len, n_hyp, scores, res = attention_beam_search(
                model, enc, mask, beam_size, 64 if max_len is None else max_len, length_penalty,
                {"blank": blank_id})
        out, cnt = hyp[:, 0].contiguous(), hyp_len[:, 0].contiguous()
        if info is not None:
            info.update(res, hyp=hyp, hyp_len=hyp_len, n_hyp=n_hyp, score=scores, enc=enc,
                        mask=mask)
        totals, map_k = scores, None  # entry 0 is the search's best
    elif decoder == "rescore":
        hyp, hyp_len, n_hyp, scores = ctc_beam_search_nbest_device(logits, lens, beam_size, None,
                                                                   blank_id)
        out, cnt, res = attention_rescore(model, enc, mask, hyp, hyp_len, n_hyp, scores,
                                          ctc_weight, max_len, {"blank": blank_id}, lm, lm_weight)
        if info is not None:
            info.update(res, hyp=hyp, hyp_len=hyp_len, n_hyp=n_hyp, ctc_scores=scores, enc=enc,
                        mask=mask)
        totals, map_k = res["total"], res["best_k"]
    elif use_bias:
        hyp, hyp_len, n_hyp, res = ctc_beam_search_bias_device(
            logits, lens, bias, float(bias_weight), lm if use_lm else None,
            lm_weight if use_lm else 0.0, ins_bonus, beam_size, None, blank_id)
        out, cnt = hyp[:, 0].contiguous(), hyp_len[:, 0].contiguous()
        if info is not None:
            info.update(hyp=hyp, hyp_len=hyp_len, n_hyp=n_hyp, ctc_scores=res["ctc"],
                        lm=res["lm"], bias=res["bias"], total=res["total"],
                        best_k=torch.zeros_like(n_hyp))
        totals, map_k = res["total"], None
    elif first_pass:
        hyp, hyp_len, n_hyp, res = ctc_beam_search_lm_device(logits, lens, lm, lm_weight, ins_bonus,
                                                             beam_size, None, blank_id)
        out, cnt = hyp[:, 0].contiguous(), hyp_len[:, 0].contiguous()
        if info is not None:
            info.update(hyp=hyp, hyp_len=hyp_len, n_hyp=n_hyp, ctc_scores=res["ctc"],
                        lm=res["lm"], total=res["total"], best_k=torch.zeros_like(n_hyp))
        totals, map_k = res["total"], None
    elif decoder == "beam" and use_lm:
        hyp, hyp_len, n_hyp, scores = ctc_beam_search_nbest_device(logits, lens, beam_size, None,
                                                                   blank_id)
        out, cnt, res = ctc_lm_rescore(hyp, hyp_len, n_hyp, scores, lm, lm_weight,
                                       logits.shape[-1], {"blank": blank_id})
        if info is not None:
            info.update(res, hyp=hyp, hyp_len=hyp_len, n_hyp=n_hyp, ctc_scores=scores)
        totals, map_k = res["total"], res["best_k"]
    elif decoder == "beam" and mbr_scale is not None:
        hyp, hyp_len, n_hyp, totals = ctc_beam_search_nbest_device(logits, lens, beam_size, None,
                                                                   blank_id)
        info.update(hyp=hyp, hyp_len=hyp_len, n_hyp=n_hyp, ctc_scores=totals)
        map_k = None
    elif decoder == "beam":
        out, cnt, _ = ctc_beam_search_batch_device(logits, lens, beam_size, blank_id)
    else:
        out, cnt = ctc_greedy_decode_batch(logits, lens, blank_id)
    if mbr_scale is not None:
        from .edit import mbr_select

        out, cnt, res = mbr_select(hyp, hyp_len, n_hyp, totals, mbr_scale)
        info.update(best_k=res["best_k"], mbr_risk=res["risk"], mbr_post=res["post"],
                    map_k=torch.zeros_like(res["best_k"]) if map_k is None else map_k)
    if timestamps:
        from .align import MAX_TARGET_LEN, ctc_forced_align

        al = ctc_forced_align(logits, lens, out, cnt, blank_id, MAX_TARGET_LEN)
        if info is not None:
            info.update(span=al.span, tok_score=al.tok_score, align_score=al.score,
                        frame_path=al.path)
    return out, cnt, logits


class GraphedInference:
    """Forward + decode for a fixed padded batch shape, captured once as a HIP graph.
    ``run(batch)`` copies the batch into the captured inputs and replays. With ``frontend`` (a
    ``FrontEnd``, put in eval mode here) the batch holds ``wave`` / ``wave_lens`` and the feature
    kernel is part of the captured graph; the padded shape is fixed by ``wave.shape``. With
    ``timestamps=True`` the forced alignment of the decoder's output is part of the graph too and
    ``self.info`` holds span / tok_score / align_score / frame_path for every decoder. With
    ``mbr_scale`` the pairwise distances and the minimum-Bayes-risk pick are part of the graph."""

    def __init__(self, model, precision: int = 2, act_quant: Optional[str] = "absmax_int8",
                 blank_id: int = 3, use_graph: bool = True, decoder: str = "greedy",
                 beam_size: int = 10, frontend=None, ctc_weight: float = 0.5,
                 max_len: int = 64, length_penalty: float = 0.0, timestamps: bool = False, *,
                 mbr_scale: Optional[float] = None, bias=None, bias_weight: float = 0.0,
                 lm=None, lm_weight: float = 0.0, lm_fusion: str = "rescore",
                 ins_bonus: float = 0.0, joint_ctc_weight: float = 0.0,
                 ctc_cand: Optional[int] = None):
        if decoder not in DECODERS:
            raise ValueError("decoder must be 'greedy', 'beam', 'rescore' or 'attention', got "
                             f"{decoder!r}")
        _check_joint(decoder, joint_ctc_weight)
        _check_timestamps(timestamps)
        self.use_lm = _check_lm(decoder, lm, lm_weight)  # n-gram shallow fusion takes part
        self.lm = lm
        self.lm_weight = float(lm_weight)
        first_pass = _check_fusion(decoder, self.use_lm, lm_fusion, ins_bonus)
        _check_bias(decoder, bias, bias_weight, self.use_lm, first_pass)
        self.bias = bias  # a ContextBias: phrase-list biasing inside the beam searches
        self.bias_weight = float(bias_weight)
        self.lm_fusion = lm_fusion  # "first_pass": the LM inside the CTC prefix beam search
        self.ins_bonus = float(ins_bonus)
        self.mbr_scale = _check_mbr(decoder, mbr_scale)  # a float: the MBR pick from the n-best
        self.timestamps = timestamps  # True: info also holds the forced alignment (any decoder)
        self.joint_ctc_weight = float(joint_ctc_weight)  # attention: > 0 = the joint search
        self.ctc_cand = ctc_cand
        self.ctc_weight = ctc_weight
        self.length_penalty = length_penalty
        self.max_len = int(max_len)  # rescore / attention: the static length of the graph
        self.info: dict = {}  # rescore / attention: what encode_and_decode's info receives
        self.frontend = frontend.eval() if frontend is not None else None
        self.decoder = decoder
        self.beam_size = beam_size
        self.model = model.eval()
        set_act_quant(self.model, act_quant)
        self.precision = precision
        self.blank_id = blank_id
        self.use_graph = use_graph
        self.graph = None
        self.inputs = None
        self.outputs = None

    def _body(self):
        # one form for every decoder: "greedy" and "beam" without an LM or timestamps read none of
        # ctc_weight / max_len / length_penalty and leave info empty, and __init__ has checked
        # that joint_ctc_weight is 0 for them
        self.info = {}
        return encode_and_decode(self.model, self.inputs, self.precision, self.blank_id,
                                 self.decoder, self.beam_size, self.frontend, self.ctc_weight,
                                 self.max_len, self.info, self.length_penalty,
                                 timestamps=self.timestamps, mbr_scale=self.mbr_scale,
                                 bias=self.bias, bias_weight=self.bias_weight, lm=self.lm,
                                 lm_weight=self.lm_weight,
                                 lm_fusion=self.lm_fusion, ins_bonus=self.ins_bonus,
                                 joint_ctc_weight=self.joint_ctc_weight, ctc_cand=self.ctc_cand)

    def run(self, batch: Dict[str, torch.Tensor]):
        if self.inputs is None:
            self.inputs = {k: v.clone() for k, v in batch.items()}
            if not self.use_graph:
                return self._body()
            side = torch.cuda.Stream(batch["feats" if self.frontend is None else "wave"].device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):  # warm-up: packs codes, picks kernels, allocates
                    self._body()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.outputs = self._body()
        else:
            for k, v in batch.items():
                if self.inputs[k].shape != v.shape:
                    raise ValueError(f"batch[{k!r}] shape {tuple(v.shape)} != captured "
                                     f"{tuple(self.inputs[k].shape)}")
                if self.inputs[k].data_ptr() != v.data_ptr():
                    self.inputs[k].copy_(v, non_blocking=True)
            if not self.use_graph:
                return self._body()
        self.graph.replay()
        return self.outputs
