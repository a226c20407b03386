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
  ``ob_ctc_beam_search`` (csrc/beam.hip);
* ``GraphedInference`` captures forward + decode as one HIP graph for a fixed padded shape;
* ``frontend=FrontEnd(...)`` (onebit_asr/frontend.py) puts the feature kernel ahead of the
  encoder: the batch then carries ``wave`` / ``wave_lens`` in place of ``feats`` / ``feat_lens``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .quant import set_act_quant

__all__ = ["ctc_greedy_decode_batch", "ctc_greedy_decode", "ctc_beam_search_batch_device",
           "GraphedInference", "encode_and_decode"]


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


MAX_BEAM = 32   # ob_ctc_beam_search's argument limits (include/onebit_hip.h)
MAX_TOP_K = 64


def ctc_beam_search_batch_device(logits: torch.Tensor, lens: torch.Tensor, beam_size: int = 10,
                                 blank_id: int = 3, top_k_per_t: Optional[int] = 20
                                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CTC prefix beam search of metrics.py:74-145 for a whole padded batch on the device.
    logits [B, T, V] fp32 (device), lens [B] valid frames -> (tokens int32 [B, T], padded with
    -1; counts int32 [B]; scores float64 [B], the log-probability of each returned prefix).
    ``top_k_per_t=None`` means every token and needs V <= 64. No host synchronisation; the
    workspace comes from the caching allocator."""
    if not logits.is_cuda:
        raise RuntimeError("ctc_beam_search_batch_device runs on the HIP library (no CPU fallback)")
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
    x = logits.contiguous().float()
    ln = lens.to(device=x.device, dtype=torch.int64).contiguous()
    out = torch.empty((b, t), dtype=torch.int32, device=x.device)
    cnt = torch.empty((b,), dtype=torch.int32, device=x.device)
    score = torch.empty((b,), dtype=torch.float64, device=x.device)
    lib = _lib.load()
    need = lib.ob_ctc_beam_search_workspace(b, t, v, beam_size, top_k)
    if b > 0 and need == 0:
        raise ValueError(f"ctc beam search: shape B={b} T={t} V={v} is not supported")
    ws = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=x.device)
    _lib.check(lib.ob_ctc_beam_search(x.data_ptr(), ln.data_ptr(), b, t, v, blank_id, beam_size,
                                      top_k, ws.data_ptr(), ws.numel() * 8, out.data_ptr(),
                                      cnt.data_ptr(), score.data_ptr(), _lib.stream_of(x)),
               "ob_ctc_beam_search")
    return out, cnt, score


@torch.no_grad()
def encode_and_decode(model, batch: Dict[str, torch.Tensor], precision: int = 2,
                      blank_id: int = 3, decoder: str = "greedy", beam_size: int = 10,
                      frontend=None):
    """Encoder + CTC head + decode of one padded batch (eval.py:118-124 for one precision).
    ``decoder="greedy"`` (the default) or ``"beam"``, the reference's beam search with its
    eval settings (beam_size, the 20 best tokens per frame). With ``frontend`` (a ``FrontEnd``)
    the batch holds ``wave`` [B, n_max] and ``wave_lens`` [B] and the features are computed
    here, on the same stream; its other entries (``tokens``...) pass through.
    Returns (tokens, counts, logits)."""
    if decoder not in ("greedy", "beam"):
        raise ValueError(f"decoder must be 'greedy' or 'beam', got {decoder!r}")
    if frontend is not None:
        rest = {k: v for k, v in batch.items() if k not in ("wave", "wave_lens")}
        batch = {**rest, **frontend(batch["wave"], batch["wave_lens"])}
    _, mask, logits = model(batch, precision=precision)
    lens = mask.sum(dim=1)
    if decoder == "beam":
        out, cnt, _ = ctc_beam_search_batch_device(logits, lens, beam_size, blank_id)
    else:
        out, cnt = ctc_greedy_decode_batch(logits, lens, blank_id)
    return out, cnt, logits


class GraphedInference:
    """Forward + decode for a fixed padded batch shape, captured once as a HIP graph.
    ``run(batch)`` copies the batch into the captured inputs and replays. With ``frontend`` (a
    ``FrontEnd``, put in eval mode here) the batch holds ``wave`` / ``wave_lens`` and the feature
    kernel is part of the captured graph; the padded shape is fixed by ``wave.shape``."""

    def __init__(self, model, precision: int = 2, act_quant: Optional[str] = "absmax_int8",
                 blank_id: int = 3, use_graph: bool = True, decoder: str = "greedy",
                 beam_size: int = 10, frontend=None):
        if decoder not in ("greedy", "beam"):
            raise ValueError(f"decoder must be 'greedy' or 'beam', got {decoder!r}")
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
        return encode_and_decode(self.model, self.inputs, self.precision, self.blank_id,
                                 self.decoder, self.beam_size, self.frontend)

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
