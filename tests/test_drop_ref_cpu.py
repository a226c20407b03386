"""The restated dropout keep-hash (tests/layernorm_ref.py) against itself: the Python-int and
the numpy versions agree, the murmur3 finaliser's known values, the threshold, the keep rate.
(tests/test_layernorm_family_gpu.py compares the device hash with the numpy version.)"""
import numpy as np
import pytest

import layernorm_ref as R

_STREAMS = [(77, 14), (0, 0), (12345, 7), (2**40 + 3, 7), (12345, 2**33 + 1),
            (2**63 + 5, 2**64 - 1)]


@pytest.mark.parametrize("seed,ctr", _STREAMS)
def test_scalar_and_numpy_versions_agree(seed, ctr):
    # 10^5 indices: a low run, a run across pair index 2^32 (element index 2^33), a run far
    # above it, and random 63-bit indices
    n = 25_000
    rng = np.random.default_rng(seed % 1000 + 1)
    idx = np.concatenate([
        np.arange(n, dtype=np.uint64),
        np.arange(n, dtype=np.uint64) + np.uint64(2**33 - n // 2),
        np.arange(n, dtype=np.uint64) + np.uint64(5 * 2**33 + 2**20 + 1),
        rng.integers(0, 2**63, n, dtype=np.uint64),
    ])
    assert int(idx.max() >> np.uint64(1)) >= 2**32
    for p in (0.1, 0.5):
        a = np.array(R.keep_scalar(seed, ctr, idx.tolist(), p))
        b = R.np_keep(seed, ctr, idx, p)
        assert np.array_equal(a, b), (seed, ctr, p, int((a != b).sum()))
    assert int(R.np_drop_key(seed, ctr)) == R.drop_key(seed, ctr)


def test_high_words_matter():
    """seed, ctr and index bits above 2^32 change the draw (they are folded in, not dropped)."""
    idx = np.arange(4096, dtype=np.uint64)
    base = R.np_keep(12345, 7, idx, 0.5)
    assert not np.array_equal(base, R.np_keep(12345 + 2**32, 7, idx, 0.5))
    assert not np.array_equal(base, R.np_keep(12345, 7 + 2**32, idx, 0.5))
    assert not np.array_equal(base, R.np_keep(12345, 7, idx + np.uint64(2**33), 0.5))
    # ... and the high-word fold is a rotate by 16, so pair 2^32 collides with pair 2^16
    assert R.drop_hash(99, 2**32) == R.drop_hash(99, 2**16)
    assert R.drop_hash(99, 2**48) == R.drop_hash(99, 1)


def test_fmix32_known_values():
    assert R.fmix32(0) == 0
    assert R.fmix32(1) == 0x514E28B7
    assert R.fmix32(0xFFFFFFFF) == 0x81F16F39
    v = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32)
    assert R._np_fmix32(v).tolist() == [0, 0x514E28B7, 0x81F16F39]


def test_thresh():
    assert R.drop_thresh(0.1) == 6554
    assert R.drop_thresh(0.5) == 32768
    assert R.drop_thresh(0.0) == 0
    assert R.drop_thresh(1.0) == 65536
    assert R.drop_thresh(2.0) == 65536


def test_p_zero_keeps_everything_and_p_one_nothing():
    idx = np.arange(10_000, dtype=np.uint64)
    assert R.np_keep(77, 14, idx, 0.0).all()
    assert all(R.keep_scalar(77, 14, range(1000), 0.0))
    assert not R.np_keep(77, 14, idx, 1.0).any()
    assert not any(R.keep_scalar(77, 14, range(1000), 1.0))


def test_keep_rate():
    n = 200_000
    rate = float(np.mean(R.keep_scalar(77, 14, range(n), 0.1)))
    print(f"keep rate seed 77 ctr 14 p 0.1: {rate:.4f}")
    assert abs(rate - 0.9) <= 0.003, rate
    for seed, ctr in _STREAMS[1:]:
        r = float(R.np_keep_flat(seed, ctr, n, 0.1).mean())
        assert abs(r - 0.9) <= 0.003, (seed, ctr, r)


def test_row_pitch():
    """np_keep_rows pads an odd row length to even; an even one is the flat index."""
    assert np.array_equal(R.np_keep_rows(5, 6, 6, 8, 0.5).ravel(), R.np_keep_flat(5, 6, 48, 0.5))
    odd = R.np_keep_rows(5, 6, 7, 5, 0.5)
    flat = R.np_keep_flat(5, 6, 7 * 6, 0.5).reshape(7, 6)
    assert np.array_equal(odd, flat[:, :5])
