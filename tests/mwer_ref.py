"""Test helper (not a test): the reference of the minimum-WER loss over the CTC n-best
(``onebit_asr.mwer``, csrc/ctcnbest.hip). Plain torch on the CPU, in the dtype of ``logits``
(float64 for the reference; float32 to measure what fp32 arithmetic alone costs), the
gradient by autograd.

``nbest_ll``: per utterance ``log_softmax`` of its valid frames, then ``F.ctc_loss(...,
reduction="none")`` per entry; ll = -nll, -inf for an entry CTC cannot align (nll = inf), for
absent entries k >= n_hyp[b] and for every entry of an utterance without frames.

``mwer``: live = k < n_hyp[b] and ll finite; over the live entries of an utterance with at
least two of them post = softmax(scale * ll), risk = sum post * err, loss_b = risk - mean(err);
otherwise loss_b = 0 (post 1 on a single live entry); loss = sum_b loss_b / B.

``token_errors``: the entries' edit distances to the references, from tests/edit_ref.py.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from edit_ref import edit_distance_np


def entries(hyp, hyp_len, n_hyp):
    """[[tokens of entry k] for k < n_hyp[b]] per utterance, from the decoders' layout."""
    return [[[int(v) for v in hyp[b, k, :int(hyp_len[b, k])]] for k in range(int(n_hyp[b]))]
            for b in range(hyp.shape[0])]


def token_errors(hyp, hyp_len, n_hyp, ref, ref_len) -> torch.Tensor:
    """float64 [B, N]: edit distance of every present entry to its reference (-1 for absent)."""
    err = torch.full(tuple(hyp_len.shape), -1.0, dtype=torch.float64)
    for b, ents in enumerate(entries(hyp, hyp_len, n_hyp)):
        r = [int(v) for v in ref[b, :int(ref_len[b])]]
        for k, e in enumerate(ents):
            err[b, k] = edit_distance_np(r, e)
    return err


def nbest_ll(logits, lens, hyp, hyp_len, n_hyp, blank) -> torch.Tensor:
    """ll [B, N] in logits' dtype, differentiable w.r.t. ``logits`` [B, T, V]."""
    B, N = hyp_len.shape
    ninf = torch.tensor(float("-inf"), dtype=logits.dtype)
    rows = []
    for b, ents in enumerate(entries(hyp, hyp_len, n_hyp)):
        tb = int(lens[b])
        row = [ninf] * N
        if tb > 0 and ents:
            lp = F.log_softmax(logits[b, :tb], dim=-1).unsqueeze(1)  # [Tb, 1, V]
            for k, e in enumerate(ents):
                tg = torch.tensor([e], dtype=torch.long).reshape(1, len(e))
                args = (tg, torch.tensor([tb]), torch.tensor([len(e)]))
                with torch.no_grad():
                    feasible = torch.isfinite(F.ctc_loss(lp, *args, blank=blank,
                                                         reduction="none"))[0]
                if feasible:
                    row[k] = -F.ctc_loss(lp, *args, blank=blank, reduction="none")[0]
        rows.append(torch.stack(row))
    return torch.stack(rows)


def mwer(ll, err, n_hyp, scale):
    """-> (loss, post [B, N], risk [B]) in ll's dtype, differentiable w.r.t. ``ll``."""
    B, N = ll.shape
    err = err.to(ll.dtype)
    total = torch.zeros((), dtype=ll.dtype)
    post = torch.zeros(B, N, dtype=ll.dtype)
    risk = torch.zeros(B, dtype=ll.dtype)
    for b in range(B):
        live = [k for k in range(int(n_hyp[b])) if torch.isfinite(ll[b, k])]
        if not live:
            continue
        p = torch.softmax(scale * ll[b, live], dim=0)
        r = (p * err[b, live]).sum()
        post[b, live] = p.detach()
        risk[b] = r.detach()
        if len(live) >= 2:
            total = total + (r - err[b, live].mean())
    return total / B, post, risk


def mwer_loss(logits, lens, hyp, hyp_len, n_hyp, err, blank, scale):
    """The composite: (loss, {ll, post, risk}) in logits' dtype."""
    ll = nbest_ll(logits, lens, hyp, hyp_len, n_hyp, blank)
    loss, post, risk = mwer(ll, err, n_hyp, scale)
    return loss, {"ll": ll.detach(), "post": post, "risk": risk}


def label_columns(hyp, hyp_len, n_hyp, blank, V) -> torch.Tensor:
    """bool [B, V]: blank and every token of the utterance's present entries."""
    m = torch.zeros(hyp.shape[0], V, dtype=torch.bool)
    m[:, blank] = True
    for b, ents in enumerate(entries(hyp, hyp_len, n_hyp)):
        for e in ents:
            for v in e:
                m[b, v] = True
    return m
