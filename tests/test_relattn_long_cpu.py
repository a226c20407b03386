"""The long-utterance attention forward's C ABI without a GPU: the header declares the three
entries and the library exports them, the getters answer, and ob_relattn_infer refuses bad
shapes and null pointers before any device call (so these run where no device exists). The
Python entry refuses CPU tensors."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "onebit_hip.h"
ENTRIES = ("ob_relattn_infer", "ob_relattn_infer_key_chunk", "ob_relattn_infer_max_t")


def _code(name):
    m = re.search(rf"\b{name}\s*=\s*(-?\d+)", HEADER.read_text())
    assert m, f"{name} not in the header"
    return int(m.group(1))


@pytest.fixture(scope="module")
def lib():
    from onebit_asr import _lib

    return _lib.load()


def test_header_declares_and_library_exports(lib):
    from onebit_asr import _lib

    text = HEADER.read_text()
    for name in ENTRIES:
        assert re.search(rf"OB_API\s+\w+\s+{name}\s*\(", text), f"{name} not declared"
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None


def test_getters(lib):
    kc = lib.ob_relattn_infer_key_chunk()
    assert kc >= 16 and kc % 16 == 0
    assert lib.ob_relattn_infer_max_t() == 4096
    from onebit_asr import attention as at

    assert at.long_key_chunk() == kc
    assert at.LONG_MAX_T == 4096
    for name in ("rel_pos_attention_infer", "LONG_MAX_T", "long_key_chunk"):
        assert name in at.__all__


def _call(lib, bt, P, t, H, d, null_ctx=False):
    # non-null dummy host pointers: validation must answer before anything reads them
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    return lib.ob_relattn_infer(p, p, p, p, p, p, p, bt, P, t, H, d, None if null_ctx else p, None)


@pytest.mark.parametrize("bt,P,t,H,d", [
    (1, 1, 0, 4, 36),      # T = 0
    (1, 1, 4097, 4, 36),   # T past the cap
    (1, 1, 600, 4, 24),    # a head width the kernel is not built for
    (3, 2, 600, 4, 36),    # Bt not a multiple of P
    (1, 1, 600, 0, 36),    # H = 0
])
def test_bad_shapes_refused(lib, bt, P, t, H, d):
    assert _call(lib, bt, P, t, H, d) == _code("OB_ERR_SHAPE")


def test_null_ctx_refused(lib):
    assert _call(lib, 2, 1, 600, 4, 36, null_ctx=True) == _code("OB_ERR_NULL")


def test_python_entry_refuses_cpu_tensors():
    from onebit_asr import attention as at

    q = torch.zeros(1, 8, 32)
    with pytest.raises((ValueError, RuntimeError)):
        at.rel_pos_attention_infer(q, q, q, q, torch.zeros(2, 16), torch.zeros(2, 16),
                                   torch.tensor([8], dtype=torch.int32), 2)
