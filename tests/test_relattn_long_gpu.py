"""The long-utterance attention forward (ob_relattn_infer, csrc/relattn_long.hip) through the C
ABI against the float64 restatement of the reference ops (relattn_ref.ref), at the project's
ctx bar (relattn_ref.CTX_BAR, unchanged).

Every call: ctx is NaN before it, 64 sentinel floats follow ctx and must come back unchanged,
the result holds no NaN, and rows >= lens[b] are exactly 0 (compared as int32). For T <= 512
the same case also runs ob_relattn_fwd (saved = NULL, p = 0): both kernels meet the bar against
float64; they need not be equal to each other.

Shapes (KC = ob_relattn_infer_key_chunk(), a query tile is 64 rows, a key tile 16 keys):
  T = 1, 15, 16, 17, 64, 65            one chunk; key-tile and query-tile edges; the query of
                                       the tile below absent and present
  T = 512, 513, 529, 576, 577          the other kernel's cap and the first lengths past it
  T = KC-1, KC, KC+1, 2KC-1, 2KC, 2KC+1  chunk edges; a last chunk of one key
  T = 3KC + 40                         chunks wholly below, on and above a tile's diagonal
  T = 1025, T = 4096                   one case each
crossed at d = 36 with (Bt, P) = (1, 1), (4, 2), H = 1 and 4, and full lengths or one of two
ragged sets that between them hold 0, 1, T, T-1, KC, KC+1, a length inside the diagonal chunk of
a middle query tile, and 70 (dead chunks and dead query tiles in a long T). Three combinations
at each of d = 16, 32, 64.

Online-softmax stress at T = 2KC+1 and 1025, d = 16 and 36: 64 consecutive rows of k times 6,
placed in the first chunk, at the end, and across the first chunk edge, so the running max moves
early, late and across an edge and whole chunks underflow to 0 against it. Same bar.
"""
import pytest
import torch

import relattn_ref as R

pytestmark = pytest.mark.gpu

SENT = -7777.0
N_GUARD = 64


@pytest.fixture(scope="module")
def lib(gpu):
    from onebit_asr import _lib

    return _lib.load()


def _kc():
    from onebit_asr import _lib

    return int(_lib.load().ob_relattn_infer_key_chunk())


KC = _kc()  # the shapes follow the library's chunk

T_SMALL = [1, 15, 16, 17, 64, 65, 512, 513, 529, 576, 577,
           KC - 1, KC, KC + 1, 2 * KC - 1, 2 * KC, 2 * KC + 1, 3 * KC + 40]
T_SMALL = list(dict.fromkeys(T_SMALL))  # duplicates removed, order kept


def _mid(t):
    """A length inside the diagonal chunk of a middle query tile (the tile stays live)."""
    i0 = 64 * (((t + 63) // 64) // 2)
    return min(t, i0 + 37)


def _lens(kind, bt, t):
    if kind == "full":
        return [t] * bt
    pool = {"ragA": [t - 1, 0, 1, _mid(t)], "ragB": [KC + 1, KC, 70, t]}[kind]
    pool = [max(0, min(x, t)) for x in pool]
    return pool[:bt] if bt > 1 else [pool[3] if kind == "ragA" else pool[0]]


class Guarded:
    """n floats followed by 64 sentinel floats."""

    def __init__(self, shape, gpu):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(n + N_GUARD, device=gpu)
        self.buf[n:] = SENT
        self.t = self.buf[:n].view(*shape)
        self.n = n

    def nan(self):
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[self.n:] == SENT).all().item())


def _infer(lib, gpu, dev, lens_d, H):
    from onebit_asr import _lib

    q, k, v, pos, u, vb = dev
    bt, t, c = q.shape
    out = Guarded((bt, t, c), gpu)
    out.nan()
    _lib.check(lib.ob_relattn_infer(q.data_ptr(), k.data_ptr(), v.data_ptr(), pos.data_ptr(),
                                    u.data_ptr(), vb.data_ptr(), lens_d.data_ptr(), bt,
                                    pos.size(0), t, H, c // H, out.t.data_ptr(), _lib.stream_of(q)),
               "ob_relattn_infer")
    torch.cuda.synchronize()
    return out


def _fwd(lib, gpu, dev, lens_d, H):
    from onebit_asr import _lib

    q, k, v, pos, u, vb = dev
    bt, t, c = q.shape
    out = Guarded((bt, t, c), gpu)
    out.nan()
    _lib.check(lib.ob_relattn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), pos.data_ptr(),
                                  u.data_ptr(), vb.data_ptr(), lens_d.data_ptr(), bt, pos.size(0),
                                  t, H, c // H, 0.0, None, 0, None, None, out.t.data_ptr(),
                                  _lib.stream_of(q)),
               "ob_relattn_fwd")
    torch.cuda.synchronize()
    return out


def _buffer_checks(out, lens, what):
    assert out.intact(), f"{what}: wrote past ctx"
    got = out.t.cpu()
    assert not torch.isnan(got).any(), f"{what}: NaN in ctx"
    for b, n in enumerate(lens):
        assert not got[b, n:].contiguous().view(torch.int32).any(), f"{what}: row >= lens[{b}] not 0"
    return got


def _check(lib, gpu, host, lens, H, what):
    q = host[0]
    t = q.size(1)
    lens_t = torch.tensor(lens, dtype=torch.int64)
    want, _ = R.ref(*(x.double() for x in host), lens_t, H)
    dev = tuple(x.to(gpu) for x in host)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=gpu)
    got = _buffer_checks(_infer(lib, gpu, dev, lens_d, H), lens, what)
    R.close(got, want, R.CTX_BAR, f"{what} ctx")
    if t <= 512:
        old = _buffer_checks(_fwd(lib, gpu, dev, lens_d, H), lens, what + " (ob_relattn_fwd)")
        R.close(old, want, R.CTX_BAR, f"{what} ctx (ob_relattn_fwd)")


@pytest.mark.parametrize("kind", ["full", "ragA", "ragB"])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("bt,P", [(1, 1), (4, 2)])
@pytest.mark.parametrize("t", T_SMALL)
def test_long_matches_reference(lib, gpu, t, bt, P, H, kind):
    host = R.inputs(bt, P, t, H, 36, seed=1000 + t)
    _check(lib, gpu, host, _lens(kind, bt, t), H, f"T={t} Bt={bt} P={P} H={H} {kind}")


@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("t,bt,P,H,kind", [
    (KC + 1, 4, 2, 4, "ragA"),
    (577, 1, 1, 1, "full"),
    (3 * KC + 40, 4, 2, 1, "ragB"),
])
def test_long_head_widths(lib, gpu, t, bt, P, H, kind, d):
    host = R.inputs(bt, P, t, H, d, seed=2000 + t + d)
    _check(lib, gpu, host, _lens(kind, bt, t), H, f"T={t} d={d} Bt={bt} H={H} {kind}")


def test_long_1025(lib, gpu):
    host = R.inputs(2, 2, 1025, 2, 36, seed=31)
    _check(lib, gpu, host, [1025, 700], 2, "T=1025")


def test_long_4096(lib, gpu):
    host = R.inputs(1, 1, 4096, 1, 16, seed=32)
    _check(lib, gpu, host, [4096], 1, "T=4096")


@pytest.mark.parametrize("where", ["first", "end", "edge"])
@pytest.mark.parametrize("d", [16, 36])
@pytest.mark.parametrize("t", [2 * KC + 1, 1025])
def test_online_softmax_stress(lib, gpu, t, d, where):
    q, k, v, pos, u, vb = R.inputs(1, 1, t, 2, d, seed=3000 + t + d)
    start = {"first": 5, "end": t - 64, "edge": KC - 32}[where]
    k = k.clone()
    k[:, start:start + 64] *= 6.0
    _check(lib, gpu, (q, k, v, pos, u, vb), [t], 2, f"stress T={t} d={d} {where}")


def test_two_runs_bit_identical(lib, gpu):
    t = 3 * KC + 40
    host = R.inputs(4, 2, t, 4, 36, seed=77)
    dev = tuple(x.to(gpu) for x in host)
    lens_d = torch.tensor(_lens("ragA", 4, t), dtype=torch.int32, device=gpu)
    a = _infer(lib, gpu, dev, lens_d, 4).t.clone()
    b = _infer(lib, gpu, dev, lens_d, 4).t
    assert torch.equal(a, b)
