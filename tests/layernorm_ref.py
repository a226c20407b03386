"""References for the LayerNorm kernel family (csrc/layernorm.hip): no GPU code in here.

Float64 torch functions on CPU tensors for the forward, the backward (autograd through
``F.layer_norm`` in double), the pair y2 = LN2(LN1(x)) and the GradScale output, and a
restatement of the dropout keep-hash (csrc/ob_drop.h) written from its description -- once on
Python ints, once vectorised in numpy -- so that a test's keep-mask does not come from the
device code it checks.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------
# float64 LayerNorm


def _d(t):
    return None if t is None else t.detach().double().cpu()


def ln_fwd(x, gamma, beta, eps):
    """(y, mean, rstd) in float64: biased variance, eps inside the square root."""
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    mean = x.mean(dim=1)
    var = ((x - mean[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    return y, mean, rstd


def ln_bwd(x, gamma, eps, dy, dres=None):
    """(dx, dgamma, dbeta) by autograd on F.layer_norm in float64; gamma None = weight 1
    (dgamma is then the gradient of that all-ones weight); dx += dres when given."""
    d = x.shape[1]
    xd = _d(x).requires_grad_(True)
    w = (_d(gamma) if gamma is not None else torch.ones(d, dtype=torch.float64)).requires_grad_(True)
    b = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    if x.shape[0] == 0:
        z = torch.zeros(d, dtype=torch.float64)
        return torch.zeros_like(xd), z, z.clone()
    F.layer_norm(xd, (d,), w, b, eps).backward(_d(dy))
    dx = xd.grad if dres is None else xd.grad + _d(dres)
    return dx, w.grad, b.grad


def ln_pair_fwd(x, g1, b1, eps1, g2, b2, eps2):
    """y1 = LN1(x), y2 = LN2(y1): (y1, mean1, rstd1, y2, mean2, rstd2) in float64."""
    y1, m1, r1 = ln_fwd(x, g1, b1, eps1)
    y2, m2, r2 = ln_fwd(y1, g2, b2, eps2)
    return y1, m1, r1, y2, m2, r2


def ln_pair_bwd(x, g1, b1, eps1, g2, eps2, dy, gres=None):
    """(dx, dg1, db1, dg2, db2) by float64 autograd through both LNs; gres: an extra
    gradient arriving on y1 (its residual use)."""
    d = x.shape[1]
    one = lambda: torch.ones(d, dtype=torch.float64)  # noqa: E731
    xd = _d(x).requires_grad_(True)
    w1 = (_d(g1) if g1 is not None else one()).requires_grad_(True)
    c1 = (_d(b1) if b1 is not None else torch.zeros(d, dtype=torch.float64)).requires_grad_(True)
    w2 = (_d(g2) if g2 is not None else one()).requires_grad_(True)
    c2 = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    y1 = F.layer_norm(xd, (d,), w1, c1, eps1)
    y2 = F.layer_norm(y1, (d,), w2, c2, eps2)
    out = (y2 * _d(dy)).sum()
    if gres is not None:
        out = out + (y1 * _d(gres)).sum()
    out.backward()
    return xd.grad, w1.grad, c1.grad, w2.grad, c2.grad


def row_valid(rows, T, lens):
    """bool [rows]: row r of batch b = r // T is valid iff r % T < lens[b]."""
    r = torch.arange(rows)
    return (r % T) < torch.as_tensor(lens, dtype=torch.int64)[r // T]


def grad_scale(dx, rscale, p, keep=None, lens=None, T=0):
    """dy2 = rscale * rowvalid * keep / (1 - p) * dx in float64; keep: bool [rows, d] (None:
    all kept), lens None: every row valid. p is the float32 the C ABI receives."""
    out = _d(dx).clone()
    if p > 0.0:
        out = out * torch.as_tensor(np.asarray(keep), dtype=torch.float64) / (1.0 - float(np.float32(p)))
    if lens is not None:
        out = out * row_valid(out.shape[0], T, lens).double()[:, None]
    return out * float(rscale)


# ---------------------------------------------------------------------------------------
# the dropout keep-hash, restated
#
# keep(i): one 32-bit hash per element PAIR i >> 1, keyed by (seed, ctr); element i takes the
# low 16 bits of the hash when i is even, the high 16 when odd, and is kept iff that field
# >= thresh = round(p * 2^16).

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def fmix32(x: int) -> int:
    """murmur3's 32-bit finaliser."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    x ^= x >> 16
    return x


def drop_key(seed: int, ctr: int) -> int:
    """The per-call key of a 64-bit (seed, counter); both are taken modulo 2^64."""
    seed &= _M64
    ctr &= _M64
    a = fmix32((seed >> 32) ^ 0x9E3779B9)
    b = fmix32((((ctr & _M32) * 0x27D4EB2F) + (ctr >> 32)) & _M32)
    return fmix32((seed & _M32) ^ a ^ b)


def _rot16(x: int) -> int:
    return ((x << 16) | (x >> 16)) & _M32


def drop_hash(key: int, pair_idx: int) -> int:
    """The hash of element pair ``pair_idx`` (64-bit): the high word enters rotated by 16."""
    pair_idx &= _M64
    return fmix32((pair_idx & _M32) ^ _rot16(pair_idx >> 32) ^ key)


def drop_thresh(p: float) -> int:
    """round(p * 2^16), capped at 2^16; p as the float32 the C ABI carries."""
    return min(int(float(np.float32(p)) * 65536.0 + 0.5), 65536)


def drop_keep(key: int, i: int, thresh: int) -> bool:
    h = drop_hash(key, i >> 1)
    return ((h >> 16) if (i & 1) else (h & 0xFFFF)) >= thresh


def keep_scalar(seed: int, ctr: int, idx, p: float):
    """[bool] for the element indices ``idx``, on Python ints."""
    key, th = drop_key(seed, ctr), drop_thresh(p)
    return [drop_keep(key, int(i), th) for i in idx]


def _np_fmix32(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def np_drop_key(seed: int, ctr: int) -> np.uint32:
    s = np.array([seed & _M64], dtype=np.uint64)
    c = np.array([ctr & _M64], dtype=np.uint64)
    lo = lambda v: (v & np.uint64(_M32)).astype(np.uint32)  # noqa: E731
    hi = lambda v: (v >> np.uint64(32)).astype(np.uint32)  # noqa: E731
    a = _np_fmix32(hi(s) ^ np.uint32(0x9E3779B9))
    b = _np_fmix32(lo(c) * np.uint32(0x27D4EB2F) + hi(c))
    return _np_fmix32(lo(s) ^ a ^ b)[0]


def np_keep(seed: int, ctr: int, idx, p: float) -> np.ndarray:
    """bool array, the keep bits of the uint64 element indices ``idx`` (any shape)."""
    idx = np.asarray(idx, dtype=np.uint64)
    key = np_drop_key(seed, ctr)
    pair = idx >> np.uint64(1)
    lo = (pair & np.uint64(_M32)).astype(np.uint32)
    hi = (pair >> np.uint64(32)).astype(np.uint32)
    h = _np_fmix32(lo ^ ((hi << np.uint32(16)) | (hi >> np.uint32(16))) ^ key)
    odd = (idx & np.uint64(1)).astype(bool)
    field = np.where(odd, h >> np.uint32(16), h & np.uint32(0xFFFF))
    return field >= np.uint32(drop_thresh(p))


def np_keep_flat(seed: int, ctr: int, n: int, p: float, start: int = 0) -> np.ndarray:
    """Elements start .. start + n - 1 of a flat tensor (the LayerNorm / BitLinear sites)."""
    return np_keep(seed, ctr, np.arange(n, dtype=np.uint64) + np.uint64(start), p)


def np_keep_rows(seed: int, ctr: int, rows: int, T: int, p: float) -> np.ndarray:
    """[rows, T] with the attention kernels' index row * pitch + j, pitch = T rounded up to
    even (a row starts on a pair boundary)."""
    pitch = T + (T & 1)
    r = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(pitch)
    return np_keep(seed, ctr, r + np.arange(T, dtype=np.uint64)[None, :], p)
