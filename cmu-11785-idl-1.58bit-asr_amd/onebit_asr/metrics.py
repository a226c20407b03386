"""Eval metrics with the reference module's names (onebit_asr/metrics.py there), so that
eval.py:17-21's ``from onebit_asr.metrics import compute_wer, ids_to_text,
ctc_beam_search_batch`` works against this package.

The decoders run on the device: ``ctc_beam_search`` / ``ctc_beam_search_batch`` call
``ob_ctc_beam_search`` (csrc/beam.hip) through ``infer.ctc_beam_search_batch_device`` and
return Python lists as the reference does (metrics.py:74-145); ``ctc_greedy_decode`` is the
one of ``infer``. The WER helpers are host-side string work (metrics.py:7-48); ``token_error_counts``
and ``compute_wer_device`` take the distances on the device instead (``onebit_asr.edit``).
``sentencepiece`` is not imported: the processor is an argument.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .infer import (attention_rescore, ctc_beam_search_batch_device,
                    ctc_beam_search_nbest_device, ctc_greedy_decode, ctc_lm_rescore)

__all__ = ["levenshtein_distance", "compute_wer", "compute_wer_device", "token_error_counts",
           "ids_to_text", "ctc_greedy_decode",
           "ctc_beam_search", "ctc_beam_search_batch", "ctc_attention_rescore_batch",
           "word_spans", "ctc_lm_rescore_batch"]


def levenshtein_distance(ref: Sequence, hyp: Sequence) -> int:
    """Edit distance (substitute / insert / delete, cost 1 each) between two sequences."""
    prev = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        cur = [i] + [0] * len(hyp)
        for j, h in enumerate(hyp, 1):
            cur[j] = prev[j - 1] if r == h else 1 + min(prev[j], cur[j - 1], prev[j - 1])
        prev = cur
    return prev[len(hyp)]


def compute_wer(refs: Sequence[str], hyps: Sequence[str]) -> Tuple[int, int]:
    """(total word edit distance, total reference words) over paired transcripts."""
    dist = words = 0
    for r, h in zip(refs, hyps):
        rw = r.split()
        dist += levenshtein_distance(rw, h.split())
        words += len(rw)
    return dist, words


def token_error_counts(hyp: torch.Tensor, cnt: torch.Tensor, ref: torch.Tensor,
                       ref_len: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Token error counts of a padded batch on the device: hyp [B, T] / cnt [B] (a decoder's
    output) against ref [B, S] / ref_len [B] -> {dist, sub, ins, del, ref_tokens}, int64 scalars on
    the device summed over the batch (``edit.edit_distance`` with the counts); the token error
    rate is dist / ref_tokens. Lengths are clamped to the widths, as the kernel does; a pair with
    a negative length is left out. No host synchronisation."""
    from .edit import edit_distance

    dist, ops = edit_distance(ref, ref_len, hyp, cnt, ops=True)
    live = dist >= 0
    ops = torch.where(live[:, None], ops, torch.zeros_like(ops)).sum(dim=0, dtype=torch.int64)
    words = ref_len.to(device=dist.device, dtype=torch.int64).clamp(max=ref.shape[1])
    return {"dist": torch.where(live, dist, torch.zeros_like(dist)).sum(dtype=torch.int64),
            "sub": ops[0], "ins": ops[1], "del": ops[2],
            "ref_tokens": torch.where(live, words, torch.zeros_like(words)).sum()}


def compute_wer_device(refs: Sequence[str], hyps: Sequence[str], device) -> Tuple[int, int]:
    """``compute_wer`` with the distances taken on ``device``: the distinct words are numbered on
    the host and all pairs go through one ``edit.edit_distance`` call. Returns the same (total
    word edit distance, total reference words). A transcript may hold 4096 words at most."""
    from .edit import edit_distance

    ids: Dict[str, int] = {}
    rw = [[ids.setdefault(w, len(ids)) for w in r.split()] for r in refs]
    hw = [[ids.setdefault(w, len(ids)) for w in h.split()] for h in hyps]
    n = min(len(rw), len(hw))  # zip's pairing
    if n == 0:
        return 0, 0

    def pad(rows):
        out = torch.zeros((n, max(1, max(len(r) for r in rows[:n]))), dtype=torch.int32)
        for k, r in enumerate(rows[:n]):
            out[k, :len(r)] = torch.tensor(r, dtype=torch.int32)
        return out.to(device), torch.tensor([len(r) for r in rows[:n]], dtype=torch.int32,
                                            device=device)

    a, a_len = pad(rw)
    b, b_len = pad(hw)
    dist = edit_distance(a, a_len, b, b_len)
    return int(dist.sum(dtype=torch.int64).item()), sum(len(r) for r in rw[:n])


def ids_to_text(ids, spm_processor, token_offset: int = 4, pad_id: int = 0) -> str:
    """Model token ids (0 pad, 1 bos, 2 eos, 3 blank, >= token_offset: piece id + offset) to
    text: ids below the offset are dropped, the rest go to ``spm_processor.decode``."""
    if isinstance(ids, torch.Tensor):
        ids = ids.tolist()
    pieces = [int(i) - token_offset for i in ids if i >= token_offset]
    return spm_processor.decode(pieces) if pieces else ""


def word_spans(ids, span, spm_processor, token_offset: int = 4) -> List[Tuple[str, int, int]]:
    """One utterance's token ids and their frame spans [len(ids), 2] (``align.ctc_forced_align``)
    -> [(word, first frame, end frame)]: pieces (``spm_processor.id_to_piece``) are grouped into
    words at SentencePiece's word-boundary mark. Ids below the offset and tokens whose span is -1
    are skipped."""
    if isinstance(ids, torch.Tensor):
        ids = ids.tolist()
    if isinstance(span, torch.Tensor):
        span = span.tolist()
    words: List[Tuple[str, int, int]] = []
    for i, (first, end) in zip(ids, span):
        if i < token_offset or first < 0:
            continue
        piece = spm_processor.id_to_piece(int(i) - token_offset)
        if piece.startswith("▁") or not words:
            words.append((piece.lstrip("▁"), int(first), int(end)))
        else:
            w, f, _ = words[-1]
            words[-1] = (w + piece, f, int(end))
    return words


def _lists(out: torch.Tensor, cnt: torch.Tensor) -> List[List[int]]:
    out, cnt = out.cpu(), cnt.cpu().tolist()
    return [out[b, :n].tolist() for b, n in enumerate(cnt)]


def ctc_beam_search(logits: torch.Tensor, beam_size: int = 10, blank_id: int = 3,
                    top_k_per_t: Optional[int] = 20) -> List[int]:
    """metrics.py:74-132 signature: one utterance's logits [T, V] -> best prefix."""
    lens = torch.tensor([logits.size(0)], device=logits.device)
    out, cnt, _ = ctc_beam_search_batch_device(logits.unsqueeze(0), lens, beam_size, blank_id,
                                               top_k_per_t)
    return _lists(out, cnt)[0]


def ctc_beam_search_batch(logits: torch.Tensor, valid_lens: torch.Tensor, beam_size: int = 10,
                          blank_id: int = 3) -> List[List[int]]:
    """metrics.py:135-145 signature: logits [B, T, V], valid_lens [B] -> one list per sample
    (the 20 best tokens per frame, as the reference's default)."""
    out, cnt, _ = ctc_beam_search_batch_device(logits, valid_lens, beam_size, blank_id)
    return _lists(out, cnt)


def ctc_attention_rescore_batch(model, enc_out: torch.Tensor, enc_mask: torch.Tensor,
                                logits: torch.Tensor, valid_lens: torch.Tensor,
                                beam_size: int = 10, blank_id: int = 3, ctc_weight: float = 0.5,
                                max_len=None, lm=None, lm_weight: float = 0.0) -> List[List[int]]:
    """Two-pass decoding of a padded batch: the CTC beam's n-best (``beam_size`` entries, the
    20 best tokens per frame) rescored by ``model.decoder`` on the encoder output
    (``infer.attention_rescore``) -> one token list per sample, like ``ctc_beam_search_batch``.
    ``lm`` / ``lm_weight``: n-gram shallow fusion, as ``attention_rescore``'s."""
    hyp, hyp_len, n_hyp, scores = ctc_beam_search_nbest_device(logits, valid_lens, beam_size, None,
                                                               blank_id)
    out, cnt, _ = attention_rescore(model, enc_out, enc_mask, hyp, hyp_len, n_hyp, scores,
                                    ctc_weight, max_len, {"blank": blank_id}, lm, lm_weight)
    return _lists(out, cnt)


def ctc_lm_rescore_batch(logits: torch.Tensor, valid_lens: torch.Tensor, lm, lm_weight: float,
                         beam_size: int = 10, blank_id: int = 3) -> List[List[int]]:
    """The CTC beam's n-best (``beam_size`` entries, the 20 best tokens per frame) picked by
    ``ctc + lm_weight * lm`` with the n-gram LM ``lm`` (``infer.ctc_lm_rescore``) -> one token
    list per sample, like ``ctc_beam_search_batch``."""
    hyp, hyp_len, n_hyp, scores = ctc_beam_search_nbest_device(logits, valid_lens, beam_size, None,
                                                               blank_id)
    out, cnt, _ = ctc_lm_rescore(hyp, hyp_len, n_hyp, scores, lm, lm_weight, logits.shape[-1],
                                 {"blank": blank_id})
    return _lists(out, cnt)


def attention_decode_batch(model, enc_out: torch.Tensor, enc_mask: torch.Tensor,
                           beam_size: int = 10, max_len: int = 64, length_penalty: float = 0.0,
                           blank_id: int = 3) -> List[List[int]]:
    """Beam search with ``model.decoder`` on the encoder output of a padded batch
    (``attdec.attention_beam_search``) -> the best hypothesis of every sample as a token list,
    like ``ctc_attention_rescore_batch``."""
    from .attdec import attention_beam_search

    hyp, hyp_len, _, _, _ = attention_beam_search(model, enc_out, enc_mask, beam_size, max_len,
                                                  length_penalty, {"blank": blank_id})
    return _lists(hyp[:, 0], hyp_len[:, 0])


def joint_decode_batch(model, enc_out: torch.Tensor, enc_mask: torch.Tensor,
                       ctc_logits: torch.Tensor, beam_size: int = 10, max_len: int = 64,
                       ctc_weight: float = 0.3, ctc_cand: Optional[int] = None,
                       length_penalty: float = 0.0, blank_id: int = 3, lm=None,
                       lm_weight: float = 0.0) -> List[List[int]]:
    """One-pass joint CTC/attention beam search on the encoder output and the CTC logits of a
    padded batch (``attdec.joint_beam_search``) -> the best hypothesis of every sample as a token
    list, like ``attention_decode_batch`` (an utterance that ends without a hypothesis: []).
    ``lm`` / ``lm_weight``: n-gram shallow fusion, as ``joint_beam_search``'s."""
    from .attdec import joint_beam_search

    hyp, hyp_len, _, _, _ = joint_beam_search(model, enc_out, enc_mask, ctc_logits, beam_size,
                                              max_len, ctc_weight, ctc_cand, length_penalty,
                                              {"blank": blank_id}, lm, lm_weight)
    return _lists(hyp[:, 0], hyp_len[:, 0])
