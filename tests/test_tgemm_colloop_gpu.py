"""GPU: the column-looped ternary GEMM of the K = 144 swish epilogues (csrc/tgemm.hip,
tgemm_colloop_kernel) against the 64-column kernel it replaces, reached through the process-wide
switch ``ob_tgemm_set_colloop`` -- the yardstick is the unchanged kernel, not the code under test.

Bars (written here):
* new path vs switch-off: ``torch.equal`` on every output -- the byte image halves every
  product exactly and the epilogue doubles the scale, each output element accumulates
  k-chunks 0..4 with lo, mid, hi inside a chunk in both kernels, the dropout hash takes the
  absolute (row, column), and the epilogue arithmetic is the same code;
* forward ``pre`` vs the plain ``ob_bitlinear_fwd_passes``: ``torch.equal`` as well;
* shapes dispatch leaves on the 64-column kernel (N not a multiple of 64, a misaligned A,
  ``alpha_raw`` 2): the same bits with the switch on as off;
* float64 oracle (dropout off): ``pre`` within tests/test_bitlinear_passes_gpu.py's forward bar
  1e-5 * max|ref| + 1e-6; ``act`` = silu(pre) within the same bar of its own reference (silu's
  slope is at most 1.1, so ``act`` inherits the error of ``pre``, plus the few ulp of the
  epilogue's v_exp / v_rcp silu -- 1e-7 relative, two orders below the bar).

Every output buffer carries 16 guard rows behind the last pass and starts as NaN: an element
the kernel does not write fails ``torch.equal`` (NaN != NaN), a row of the clamped A prefetch
stored past M shows in the guard rows.
"""
import math

import numpy as np
import pytest
import torch

from oracle import quant_oracle as qo

pytestmark = pytest.mark.gpu

K = 144
GUARD = 16
BITS = {1: None, 3: [2, 1, 1]}


class _Case:
    """Operands of one (N, M, P): lin1 forward X [P*M, 144] -> [P*M, N] and lin2 dX
    dY [P*M, 144] -> [P*M, N] (the dX of a 144-output layer with N inputs)."""

    def __init__(self, dev, N, M, P, seed=0):
        from onebit_asr.quant import pack_codes

        g = torch.Generator(device="cpu").manual_seed(1000 * N + 10 * M + P + seed)
        rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
        self.N, self.M, self.P = N, M, P
        self.X = rnd(P * M, K)
        self.dY = rnd(P * M, K)
        self.pre_in = rnd(P * M, N)
        self.W1 = ((torch.rand(N, K, generator=g) * 2 - 1) * (2 / math.sqrt(K))).to(dev)
        self.W2 = ((torch.rand(K, N, generator=g) * 2 - 1) * (2 / math.sqrt(N))).to(dev)
        self.a1 = self.W1.abs().mean()
        self.a2 = self.W2.abs().mean()
        self.bias = rnd(N)
        self.c2, _ = pack_codes(self.W1, self.a1, 2)
        self.c1, _ = pack_codes(self.W1, self.a1, 1)
        _, self.c2t = pack_codes(self.W2, self.a2, 2)
        _, self.c1t = pack_codes(self.W2, self.a2, 1)
        self.pbits = (torch.tensor(BITS[P], dtype=torch.int32, device=dev) if BITS[P] else None)
        self.rng = torch.tensor([1234, 5], dtype=torch.int64, device=dev)

    def _out(self):
        return torch.full((self.P * self.M + GUARD, self.N), float("nan"), device=self.X.device)

    def fwd(self, lib, p_drop, X=None, codes=None, alpha_raw=1, rng_off=77):
        from onebit_asr import _lib

        X = self.X if X is None else X
        c2, c1 = (self.c2, self.c1) if codes is None else codes
        pre, act = self._out(), self._out()
        pb = self.pbits.data_ptr() if self.pbits is not None else None
        _lib.check(lib.ob_bitlinear_fwd_swish_drop(
            X.data_ptr(), self.P, self.M, K, c2.data_ptr(), c1.data_ptr(), pb, self.a1.data_ptr(),
            alpha_raw, self.bias.data_ptr(), self.N, p_drop, self.rng.data_ptr(), rng_off,
            pre.data_ptr(), act.data_ptr(), _lib.stream_of(X)), "ob_bitlinear_fwd_swish_drop")
        return pre, act

    def bwd(self, lib, p_drop, rng_off=77):
        from onebit_asr import _lib

        dpre = self._out()
        pb = self.pbits.data_ptr() if self.pbits is not None else None
        _lib.check(lib.ob_bitlinear_bwd_dx_swish_drop(
            self.dY.data_ptr(), self.P, self.M, K, self.c2t.data_ptr(), self.c1t.data_ptr(), pb,
            self.a2.data_ptr(), 1, self.N, self.pre_in.data_ptr(), p_drop, self.rng.data_ptr(),
            rng_off, dpre.data_ptr(), _lib.stream_of(self.dY)), "ob_bitlinear_bwd_dx_swish_drop")
        return (dpre,)


def _both(lib, fn):
    """fn() under the switch off, then on; the previous setting restored."""
    prev = lib.ob_tgemm_set_colloop(0)
    try:
        off = fn()
        lib.ob_tgemm_set_colloop(1)
        on = fn()
        torch.cuda.synchronize()
    finally:
        lib.ob_tgemm_set_colloop(prev)
    return off, on


def _check_same(off, on, rows):
    for a, b in zip(off, on):
        assert not torch.isnan(a[:rows]).any()  # the yardstick wrote every element
        assert torch.equal(a[:rows], b[:rows])
        assert torch.isnan(b[rows:]).all()  # nothing stored behind the last pass


def test_switch_defaults_on_and_returns_previous(gpu):
    from onebit_asr import _lib, fused

    lib = _lib.load()
    assert lib.ob_tgemm_set_colloop(-1) == 1  # query only
    assert fused.set_tgemm_colloop(False) is True
    assert lib.ob_tgemm_set_colloop(7) == 0 and lib.ob_tgemm_set_colloop(1) == 0
    assert fused.set_tgemm_colloop(True) is True


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("M", [1, 16, 17, 127, 131, 300])
@pytest.mark.parametrize("N", [64, 192, 576])
def test_bitwise_equal_to_the_64_column_kernel(gpu, N, M, P):
    from onebit_asr import _lib

    lib = _lib.load()
    case = _Case(gpu, N, M, P)
    for p_drop in (0.0, 0.1):
        off, on = _both(lib, lambda: case.fwd(lib, p_drop))
        _check_same(off, on, P * M)
        off, on = _both(lib, lambda: case.bwd(lib, p_drop))
        _check_same(off, on, P * M)


def test_pre_equals_the_plain_forward(gpu):
    from onebit_asr import _lib

    lib = _lib.load()
    N, M, P = 576, 131, 3
    case = _Case(gpu, N, M, P)
    pre, _ = case.fwd(lib, 0.1)
    Y = torch.full((P * M, N), float("nan"), device=gpu)
    _lib.check(lib.ob_bitlinear_fwd_passes(
        case.X.data_ptr(), P, M, K, case.c2.data_ptr(), case.c1.data_ptr(), case.pbits.data_ptr(),
        case.a1.data_ptr(), 1, case.bias.data_ptr(), N, Y.data_ptr(), _lib.stream_of(Y)),
        "ob_bitlinear_fwd_passes")
    torch.cuda.synchronize()
    assert torch.equal(pre[:P * M], Y)


@pytest.mark.parametrize("kind", ["n80", "misaligned_a", "alpha_raw2"])
def test_shapes_left_on_the_64_column_kernel(gpu, kind):
    from onebit_asr import _lib

    lib = _lib.load()
    M, P = 131, 3
    if kind == "n80":
        case = _Case(gpu, 80, M, P)
        off, on = _both(lib, lambda: case.fwd(lib, 0.1))
        _check_same(off, on, P * M)
        off, on = _both(lib, lambda: case.bwd(lib, 0.1))
    elif kind == "misaligned_a":
        case = _Case(gpu, 576, M, P)
        flat = torch.empty(P * M * K + 1, device=gpu)
        X = flat[1:].view(P * M, K)  # 4 bytes past a 16-byte boundary
        X.copy_(case.X)
        assert X.data_ptr() % 16 == 4
        off, on = _both(lib, lambda: case.fwd(lib, 0.1, X=X))
    else:  # quant-off: the "codes" are the bf16 weight image [N][K]
        case = _Case(gpu, 576, M, P)
        wb = case.W1.to(torch.bfloat16).contiguous()
        off, on = _both(lib, lambda: case.fwd(lib, 0.1, codes=(wb, wb), alpha_raw=2))
    _check_same(off, on, P * M)


def test_against_the_float64_oracle(gpu):
    from onebit_asr import _lib

    lib = _lib.load()
    N, M, P = 576, 131, 3
    case = _Case(gpu, N, M, P)
    pre, act = case.fwd(lib, 0.0)
    torch.cuda.synchronize()
    W = case.W1.cpu().numpy()
    araw = float(case.a1.item())
    b = case.bias.cpu().numpy()
    for p, bits in enumerate(BITS[P]):
        X = case.X[p * M:(p + 1) * M].cpu().numpy()
        ref = qo.np_bitlinear_fwd(X, W, araw, b, bits)
        ref_act = ref / (1.0 + np.exp(-ref))
        e_pre = np.abs(pre[p * M:(p + 1) * M].cpu().numpy() - ref).max()
        e_act = np.abs(act[p * M:(p + 1) * M].cpu().numpy() - ref_act).max()
        print(f"pass {p}: pre err {e_pre:.3e} (max|ref| {np.abs(ref).max():.3f}), "
              f"act err {e_act:.3e} (max|ref| {np.abs(ref_act).max():.3f})")
        assert e_pre <= 1e-5 * np.abs(ref).max() + 1e-6
        assert e_act <= 1e-5 * np.abs(ref_act).max() + 1e-6
