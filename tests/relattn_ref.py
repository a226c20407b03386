"""The float64 restatement of the relative-position attention core that the attention tests
compare against (conformer.py:115-127 with rel_shift :97-103), on the CPU with autograd, and
the bars that go with it: ctx max|err| <= 1e-5 * max|ref| + 1e-6, every gradient max|err| <=
1e-4 * max|ref| + 1e-6."""
import math

import torch

CTX_BAR = (1e-5, 1e-6)   # (relative to max|ref|, absolute)
GRAD_BAR = (1e-4, 1e-6)


def ref(q, k, v, pos, u, vb, lens, H, keep=None, p=0.0):
    """Reference ops in float64 (the oracle's gather restatement of rel_shift -- not the
    product's own). Returns (ctx, probabilities before dropout)."""
    from oracle.conformer_oracle import _rel_shift_gather as rel_shift

    bt, t, c = q.shape
    d = c // H
    P = pos.size(0)
    heads = lambda x: x.view(x.size(0), t, H, d).transpose(1, 2)  # noqa: E731
    qh, kh, vh = heads(q), heads(k), heads(v)
    ph = heads(pos)                                        # [P, H, T, d]
    ph = ph.repeat_interleave(bt // P, dim=0)              # pass of each batch row
    ac = torch.matmul(qh + u.view(1, H, 1, d), kh.transpose(-2, -1))
    bd = rel_shift(torch.matmul(qh + vb.view(1, H, 1, d), ph.transpose(-2, -1)))
    s = (ac + bd) / math.sqrt(d)
    frames = torch.arange(t)
    km = frames[None, :] < lens[:, None]
    mask = km[:, :, None] & km[:, None, :]
    s = s.masked_fill(~mask[:, None], float("-inf"))
    a = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    probs = a
    if keep is not None:
        a = a * keep.to(a.dtype) / (1.0 - p)
    ctx = torch.matmul(a, vh).transpose(1, 2).reshape(bt, t, c)
    return ctx, probs


def inputs(bt, P, t, H, d, seed):
    g = torch.Generator().manual_seed(seed)
    c = H * d
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return mk(bt, t, c), mk(bt, t, c), mk(bt, t, c), mk(P, t, c), mk(H, d) * 0.1, mk(H, d) * 0.1


def close(got, want, bar, what):
    rel, atol = bar
    err = (got.double().cpu() - want).abs().max().item() if want.numel() else 0.0
    bound = rel * (want.abs().max().item() if want.numel() else 0.0) + atol
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"
