"""Minimum-WER training over the CTC n-best (csrc/ctcnbest.hip).

* ``nbest_ctc_logprob``: the CTC log-likelihood of every entry of an n-best, straight from the
  CTC head's logits and differentiable w.r.t. them (``ob_ctc_nbest_logprob`` /
  ``ob_ctc_nbest_grad``): the primitive any n-best-level objective can be built on;
* ``mwer_ctc_loss``: the expected number of errors under the model's own posterior over its
  n-best, minus the n-best's mean (Prabhavalkar et al. 2018), as one fused autograd Function
  (``ob_mwer_combine`` in the forward, the sparse gradient in the backward).

The n-best is the decoders' layout (hyp int32 [B, N, Th], hyp_len [B, N], n_hyp [B]); the
definitions and limits are in include/onebit_hip.h. Nothing here synchronises with the host; the
workspaces come from the caching allocator; all of it, the beam search included, can be captured
in a HIP graph. There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import _lib

__all__ = ["nbest_ctc_logprob", "mwer_ctc_loss"]

MAX_NBEST = 32   # ob_ctc_nbest_supported's limits (include/onebit_hip.h)
MAX_LEN = 511


def _i32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _nbest_args(fn: str, logits, lens, hyp, hyp_len, n_hyp, blank_id):
    if not logits.is_cuda:
        raise RuntimeError(f"{fn} runs on the HIP library (no CPU fallback)")
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError(f"{fn}: logits {tuple(logits.shape)} {logits.dtype} are not float32 "
                         "[B, T, V]")
    if hyp.dim() != 3:
        raise ValueError(f"{fn}: hyp {tuple(hyp.shape)} is not [B, N, Th]")
    b, t, v = logits.shape
    n, th = hyp.shape[1], hyp.shape[2]
    if hyp.shape[0] != b or hyp_len.shape != (b, n) or n_hyp.shape != (b,) or lens.shape != (b,):
        raise ValueError(f"{fn}: hyp {tuple(hyp.shape)} / hyp_len {tuple(hyp_len.shape)} / n_hyp "
                         f"{tuple(n_hyp.shape)} / lens {tuple(lens.shape)} do not match a batch "
                         f"of {b}")
    if not _lib.load().ob_ctc_nbest_supported(n, th):
        raise ValueError(f"{fn}: N={n}, Th={th} is not supported (1 <= N <= {MAX_NBEST}, "
                         f"Th <= {MAX_LEN})")
    if b < 1 or t < 1:
        raise ValueError(f"{fn}: an empty batch or no frames (B={b}, T={t})")
    if not 0 <= blank_id < v:
        raise ValueError(f"{fn}: blank_id {blank_id} outside the vocabulary of {v}")
    dev = logits.device
    return (lens.to(device=dev, dtype=torch.int64).contiguous(), _i32(hyp, dev),
            _i32(hyp_len, dev), _i32(n_hyp, dev))


def _logprob(x, lens, hyp, hyp_len, n_hyp, blank):
    """ob_ctc_nbest_logprob on prepared arguments -> (ll float64 [B, N], the workspace)."""
    b, t, v = x.shape
    n, th = hyp.shape[1], hyp.shape[2]
    lib = _lib.load()
    need = lib.ob_ctc_nbest_workspace(b, n, t, th)
    if need == 0:
        raise ValueError(f"n-best CTC: shape B={b} N={n} T={t} Th={th} is not supported")
    ws = torch.empty((need,), dtype=torch.uint8, device=x.device)
    ll = torch.empty((b, n), dtype=torch.float64, device=x.device)
    _lib.check(lib.ob_ctc_nbest_logprob(x.data_ptr(), lens.data_ptr(), hyp.data_ptr(),
                                        hyp_len.data_ptr(), n_hyp.data_ptr(), b, n, t, v, th,
                                        blank, ws.data_ptr(), need, ll.data_ptr(),
                                        _lib.stream_of(x)), "ob_ctc_nbest_logprob")
    return ll, ws


def _grad(x, lens, hyp, hyp_len, n_hyp, blank, coef, grad_out, dense, ws):
    b, t, v = x.shape
    n, th = hyp.shape[1], hyp.shape[2]
    grad = torch.empty_like(x)  # every row is written by the kernel: no memset node
    _lib.check(_lib.load().ob_ctc_nbest_grad(
        x.data_ptr(), lens.data_ptr(), hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(), b, n,
        t, v, th, blank, coef.data_ptr(), _lib.ptr(grad_out), dense, ws.data_ptr(), ws.numel(),
        grad.data_ptr(), _lib.stream_of(x)), "ob_ctc_nbest_grad")
    return grad


class _NbestLogprobFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, lens, hyp, hyp_len, n_hyp, blank):
        x = logits.contiguous()
        ll, ws = _logprob(x, lens, hyp, hyp_len, n_hyp, blank)
        ctx.save_for_backward(x, lens, hyp, hyp_len, n_hyp, ws)
        ctx.blank = blank
        return ll

    @staticmethod
    def backward(ctx, g_ll):
        x, lens, hyp, hyp_len, n_hyp, ws = ctx.saved_tensors
        coef = g_ll.to(torch.float64).contiguous()
        return (_grad(x, lens, hyp, hyp_len, n_hyp, ctx.blank, coef, None, 1, ws),
                None, None, None, None, None)


def nbest_ctc_logprob(logits: torch.Tensor, lens: torch.Tensor, hyp: torch.Tensor,
                      hyp_len: torch.Tensor, n_hyp: torch.Tensor, blank_id: int = 3
                      ) -> torch.Tensor:
    """logits float32 [B, T, V] (the CTC head's), lens [B] valid frames, an n-best hyp [B, N, Th]
    / hyp_len [B, N] / n_hyp [B] -> ll float64 [B, N], log p_ctc(entry | logits): -inf for an
    entry CTC cannot align and for absent entries k >= n_hyp[b]. Differentiable w.r.t.
    ``logits``: the backward takes any upstream gradient of ``ll`` (entries at -inf contribute
    nothing). N <= 32, Th <= 511."""
    lens, hyp, hyp_len, n_hyp = _nbest_args("nbest_ctc_logprob", logits, lens, hyp, hyp_len, n_hyp,
                                            blank_id)
    return _NbestLogprobFn.apply(logits, lens, hyp, hyp_len, n_hyp, blank_id)


class _MwerFn(torch.autograd.Function):
    """ll, the combine and the loss in the forward; the sparse gradient (the coefficients sum
    to zero over an utterance, so the softmax terms cancel) in the backward."""

    @staticmethod
    def forward(ctx, logits, lens, hyp, hyp_len, n_hyp, err, blank, scale):
        x = logits.contiguous()
        b, n = err.shape
        ll, ws = _logprob(x, lens, hyp, hyp_len, n_hyp, blank)
        dev = x.device
        loss = torch.empty((), dtype=torch.float64, device=dev)
        post = torch.empty((b, n), dtype=torch.float64, device=dev)
        coef = torch.empty((b, n), dtype=torch.float64, device=dev)
        risk = torch.empty((b,), dtype=torch.float64, device=dev)
        _lib.check(_lib.load().ob_mwer_combine(
            ll.data_ptr(), err.data_ptr(), n_hyp.data_ptr(), scale, b, n, loss.data_ptr(),
            post.data_ptr(), risk.data_ptr(), coef.data_ptr(), _lib.stream_of(x)),
            "ob_mwer_combine")
        ctx.save_for_backward(x, lens, hyp, hyp_len, n_hyp, coef, ws)
        ctx.blank = blank
        ctx.mark_non_differentiable(ll, post, risk)
        return loss.to(torch.float32), ll, post, risk

    @staticmethod
    def backward(ctx, g_loss, _g_ll, _g_post, _g_risk):
        x, lens, hyp, hyp_len, n_hyp, coef, ws = ctx.saved_tensors
        g = g_loss.to(torch.float32).contiguous()
        return (_grad(x, lens, hyp, hyp_len, n_hyp, ctx.blank, coef, g, 0, ws),
                None, None, None, None, None, None, None)


def mwer_ctc_loss(logits: torch.Tensor, lens: torch.Tensor, ref: Optional[torch.Tensor],
                  ref_len: Optional[torch.Tensor], hyp: Optional[torch.Tensor] = None,
                  hyp_len: Optional[torch.Tensor] = None, n_hyp: Optional[torch.Tensor] = None, *,
                  beam_size: int = 10, nbest: int = 4, top_k_per_t: Optional[int] = 20,
                  blank_id: int = 3, scale: float = 1.0, errors: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The minimum-WER loss of the CTC head's ``logits`` float32 [B, T, V] (``lens`` [B] valid
    frames) over an n-best, against the references ``ref`` [B, S] / ``ref_len`` [B].

    Over the live entries of an utterance (k < n_hyp[b] with a finite CTC log-likelihood ll_k):
    post = softmax(scale * ll), risk = sum_k post_k * err_k, loss_b = risk - mean_k(err_k); an
    utterance with fewer than two live entries has loss 0. Returns (the mean of loss_b over the
    batch, float32 scalar, differentiable w.r.t. ``logits``; info).

    Without ``hyp`` / ``hyp_len`` / ``n_hyp`` the n-best is ``ctc_beam_search_nbest_device`` on
    ``logits.detach()`` (``beam_size``, ``nbest``, ``top_k_per_t``). Without ``errors`` the error
    counts are the token edit distances ``nbest_edit_distance(...)["dref"]``; ``errors`` [B, N]
    supplies other counts (word-level ones, say), and then ``ref`` / ``ref_len`` may be None.
    ``info``: ll, post, err float64 [B, N], risk float64 [B], hyp, hyp_len, n_hyp (detached)."""
    fn = "mwer_ctc_loss"
    scale = float(scale)
    if not 0 <= scale < math.inf:
        raise ValueError(f"{fn}: scale must be >= 0 and finite, got {scale}")
    if (hyp is None) != (hyp_len is None) or (hyp is None) != (n_hyp is None):
        raise ValueError(f"{fn}: hyp, hyp_len and n_hyp go together")
    if hyp is None:
        from .infer import ctc_beam_search_nbest_device

        if logits.dim() != 3:
            raise ValueError(f"{fn}: logits {tuple(logits.shape)} are not [B, T, V]")
        top_k = None if top_k_per_t is None else min(top_k_per_t, logits.shape[2])
        hyp, hyp_len, n_hyp, _ = ctc_beam_search_nbest_device(
            logits.detach(), lens, beam_size=beam_size, nbest=nbest, blank_id=blank_id,
            top_k_per_t=top_k)
        if hyp.shape[2] > MAX_LEN:  # T > 511 frames: an entry is cut at the 511 tokens CTC takes
            hyp = hyp[:, :, :MAX_LEN].contiguous()
            hyp_len = hyp_len.clamp(max=MAX_LEN)
    lens, hyp, hyp_len, n_hyp = _nbest_args(fn, logits, lens, hyp, hyp_len, n_hyp, blank_id)
    b, n = hyp_len.shape
    if errors is None:
        from .edit import nbest_edit_distance

        if ref is None or ref_len is None:
            raise ValueError(f"{fn}: ref and ref_len are needed when errors is not given")
        err = nbest_edit_distance(hyp, hyp_len, n_hyp, ref, ref_len)["dref"].to(torch.float64)
    else:
        if errors.shape != (b, n):
            raise ValueError(f"{fn}: errors {tuple(errors.shape)} do not match the n-best "
                             f"[{b}, {n}]")
        err = errors.detach().to(device=logits.device, dtype=torch.float64).contiguous()
    loss, ll, post, risk = _MwerFn.apply(logits, lens, hyp, hyp_len, n_hyp, err, blank_id, scale)
    return loss, {"ll": ll, "post": post, "err": err, "risk": risk, "hyp": hyp,
                  "hyp_len": hyp_len, "n_hyp": n_hyp}
