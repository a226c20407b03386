"""CTC forced alignment on the device (csrc/align.hip, ``ob_ctc_align``): the Viterbi path of a
token sequence through the CTC trellis of the encoder's logits -> when each token was emitted and
how sure the model is of it. It serves the output of every decoder and reference transcripts alike.

* ``ctc_forced_align``: (path, span, tok_score, score) for a padded batch, no host synchronisation;
* ``token_confidence``: the geometric mean of a token's frame posteriors over its span;
* ``span_seconds``: spans as seconds on the subsampled frame grid.

``metrics.word_spans`` groups the token spans into words on the host.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib

__all__ = ["Alignment", "ctc_forced_align", "token_confidence", "span_seconds"]

MAX_FRAMES = 4096        # ob_ctc_align's limits (include/onebit_hip.h)
MAX_TARGET_LEN = 511


class Alignment(NamedTuple):
    path: torch.Tensor       # int32 [B, T']
    span: torch.Tensor       # int32 [B, S, 2]
    tok_score: torch.Tensor  # float64 [B, S]
    score: torch.Tensor      # float64 [B]


def ctc_forced_align(logits: torch.Tensor, lens: torch.Tensor, targets: torch.Tensor,
                     target_lens: torch.Tensor, blank_id: int = 3,
                     max_target_len: Optional[int] = None) -> Alignment:
    """logits [B, T', V] fp32 (device), lens [B] valid frames, targets [B, S] int32 or int64
    (padded with anything), target_lens [B] -> ``Alignment``:

    * path int32 [B, T']: the token emitted at frame t (``blank_id`` for a blank frame), -1 past
      ``lens`` and for an utterance without an alignment;
    * span int32 [B, S, 2]: (first frame, last frame + 1) of every token, (-1, -1) past
      ``target_lens`` and for an utterance without an alignment;
    * tok_score float64 [B, S]: the sum of the token's frame log-posteriors over its span;
    * score float64 [B]: the log-probability of the path, -inf when the target cannot be aligned
      (more tokens than frames, a repeat without room for its blank, a token outside the vocabulary
      or equal to ``blank_id``).

    Ties go to the earlier state, so a token keeps its frames as long as it can. ``max_target_len``
    narrows S (and the workspace) to the first ``max_target_len`` columns of ``targets``;
    ``target_lens`` above S are clamped to S. T' <= 4096, S <= 511. No host synchronisation; the
    workspace comes from the caching allocator; capturable in a HIP graph."""
    if not logits.is_cuda:
        raise RuntimeError("ctc_forced_align runs on the HIP library (no CPU fallback)")
    if logits.dim() != 3 or targets.dim() != 2:
        raise ValueError(f"ctc_forced_align: logits {tuple(logits.shape)} / targets "
                         f"{tuple(targets.shape)} are not [B, T', V] / [B, S]")
    b, tp, v = logits.shape
    s = targets.shape[1]
    if max_target_len is not None:
        if max_target_len < 0:
            raise ValueError(f"max_target_len must be >= 0, got {max_target_len}")
        s = min(s, int(max_target_len))
    if targets.shape[0] != b or lens.shape != (b,) or target_lens.shape != (b,):
        raise ValueError(f"ctc_forced_align: lens {tuple(lens.shape)}, targets "
                         f"{tuple(targets.shape)}, target_lens {tuple(target_lens.shape)} do not "
                         f"match a batch of {b}")
    if not 0 <= blank_id < v:
        raise ValueError(f"blank_id {blank_id} outside the vocabulary of {v}")
    lib = _lib.load()
    if not lib.ob_ctc_align_supported(tp, s):
        raise ValueError(f"ctc_forced_align: T'={tp}, S={s} is not supported "
                         f"(1 <= T' <= {MAX_FRAMES}, S <= {MAX_TARGET_LEN})")
    dev = logits.device
    x = logits.contiguous().float()
    ln = lens.to(device=dev, dtype=torch.int64).contiguous()
    tg = targets[:, :s].to(device=dev, dtype=torch.int32).contiguous()
    tl = target_lens.to(device=dev, dtype=torch.int32).contiguous()
    path = torch.empty((b, tp), dtype=torch.int32, device=dev)
    span = torch.empty((b, s, 2), dtype=torch.int32, device=dev)
    tok_score = torch.empty((b, s), dtype=torch.float64, device=dev)
    score = torch.empty((b,), dtype=torch.float64, device=dev)
    need = lib.ob_ctc_align_workspace(b, tp, s)
    if b > 0 and need == 0:
        raise ValueError(f"ctc_forced_align: shape B={b} T'={tp} S={s} is not supported")
    ws = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)
    _lib.check(lib.ob_ctc_align(x.data_ptr(), ln.data_ptr(), tg.data_ptr(), tl.data_ptr(), b, tp,
                                v, s, blank_id, ws.data_ptr(), ws.numel() * 8, path.data_ptr(),
                                span.data_ptr(), tok_score.data_ptr(), score.data_ptr(),
                                _lib.stream_of(x)), "ob_ctc_align")
    return Alignment(path, span, tok_score, score)


def token_confidence(span: torch.Tensor, tok_score: torch.Tensor) -> torch.Tensor:
    """``exp(tok_score / frames)`` as float32 [B, S], the geometric mean of the token's frame
    posteriors over its span; 0 where the span is -1."""
    frames = span[..., 1] - span[..., 0]
    valid = span[..., 0] >= 0
    conf = torch.exp(tok_score / frames.clamp(min=1)).float()
    return torch.where(valid, conf, torch.zeros_like(conf))


def span_seconds(span: torch.Tensor, frame_shift: float = 0.04
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(start, end) of every span in seconds on the subsampled frame grid: frame index x
    ``frame_shift`` (0.04 s = 10 ms features subsampled by 4), float64 like ``span`` in shape
    without its last axis; -1 where the span is -1. This ignores the subsampling's receptive
    field: a frame is taken to cover exactly its own ``frame_shift`` seconds, although the
    convolutions ahead of the encoder see some context on either side of it."""
    span = torch.as_tensor(span)
    sec = span.to(torch.float64) * float(frame_shift)
    sec = torch.where(span < 0, torch.full_like(sec, -1.0), sec)
    return sec[..., 0], sec[..., 1]
