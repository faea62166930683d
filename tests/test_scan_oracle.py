"""The two CPU references of the affine scan (tests/scan_oracle.py) agree; no GPU."""
import numpy as np
import pytest

import scan_oracle as so


def elements(n, seed=0):
    rng = np.random.default_rng([seed, n])
    return so.pack(rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint64))


@pytest.mark.parametrize("inclusive", [True, False])
@pytest.mark.parametrize("n", [0, 1, 2, 5, 4097])
def test_doubling_scan_is_the_serial_scan(n, inclusive):
    x = elements(n)
    keep = x.copy()
    serial = so.affine_scan_serial(x, inclusive)
    doubled = so.affine_scan(x, inclusive)
    assert serial.dtype == doubled.dtype == np.uint64 and len(serial) == len(doubled) == n
    assert np.array_equal(serial, doubled)
    assert np.array_equal(x, keep)                      # neither changes its input


def test_known_values_and_order():
    # x -> 2x + 1, then x -> 3x + 5: 3(2x + 1) + 5 = 6x + 8; the other order gives 2(3x + 5) + 1 = 6x + 11
    x = so.pack([2, 3], [1, 5])
    assert so.affine_scan_serial(x).tolist() == [(2 << 32) | 1, (6 << 32) | 8]
    assert so.affine_scan(x).tolist() == [(2 << 32) | 1, (6 << 32) | 8]
    assert so.affine_scan(x[::-1].copy()).tolist() == [(3 << 32) | 5, (6 << 32) | 11]
    assert so.affine_scan(x, inclusive=False).tolist() == [1 << 32, (2 << 32) | 1]
    # wrap-around modulo 2^32
    y = so.pack([0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 2])
    a, b = so.unpack(so.affine_scan(y))
    assert a.tolist() == [0xFFFFFFFF, 1] and b.tolist() == [0xFFFFFFFF, (0xFFFFFFFF * 0xFFFFFFFF + 2) & 0xFFFFFFFF]
