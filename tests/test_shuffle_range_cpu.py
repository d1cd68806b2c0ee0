"""CPU tests of the range form of the row shuffle: bear_shuffle_gather_host -- rows perm(first) .. perm(first + n_out - 1) of a
host table, gathered by host threads -- against the oracle's permutation.  Exact bytes; no device is needed."""
import ctypes

import numpy as np
import pytest

import bear_oracle as o
from bear_amd import _lib, kernels

SEEDS = (3, 20211012 << 20)
_perms = {}


def perm_of(n, seed):
    if (n, seed) not in _perms:
        _perms[(n, seed)] = np.asarray(o.shuffle_perm(n, seed), dtype=np.int64)
    return _perms[(n, seed)]


def ranges(n):
    """(first, n_out): empty (at the start, inside, at the end), whole, first > 0 up to n_rows, an interior range."""
    out = {(0, 0), (n // 2, 0), (n, 0), (0, n), (n - n // 3, n // 3), (n // 4, n // 2)}
    if n > 1:
        out |= {(1, n - 1), (n // 3, 1)}
    return sorted(out)


@pytest.mark.parametrize("n", [1, 2, 5, 1365, 4099])
@pytest.mark.parametrize("row_bytes", [1, 13, 20, 84])
def test_host_gather_matches_oracle_permutation(n, row_bytes):
    rng = np.random.default_rng(n * 100 + row_bytes)
    table = rng.integers(0, 256, size=(n, row_bytes), dtype=np.uint8)
    for seed in SEEDS:
        perm = perm_of(n, seed)
        for first, n_out in ranges(n):
            want = table[perm[first:first + n_out]]
            for n_threads in (1, 3, 16):
                got = kernels.shuffle_gather_host(table, first, n_out, seed, n_threads=n_threads)
                assert got.shape == (n_out, row_bytes) and got.dtype == np.uint8
                assert np.array_equal(got, want), (seed, first, n_out, n_threads)


def test_host_gather_keeps_shape_and_dtype_of_wider_elements():
    """A count column goes in as int32 [n, 5] or [n, 21]: the rows come back with the array's own row shape and dtype."""
    rng = np.random.default_rng(8)
    for width in (5, 21):
        table = rng.integers(-2 ** 31, 2 ** 31, size=(1365, width)).astype(np.int32)
        got = kernels.shuffle_gather_host(table, 500, 500, 7)
        assert got.dtype == np.int32 and np.array_equal(got, table[perm_of(1365, 7)[500:1000]])
    flat = rng.integers(0, 2 ** 62, size=4099)
    assert np.array_equal(kernels.shuffle_gather_host(flat, 4000, 99, 7, n_threads=64), flat[perm_of(4099, 7)[4000:]])


def test_host_gather_agrees_with_the_abi_permutation():
    table = np.arange(1365, dtype=np.int64)
    got = kernels.shuffle_gather_host(table, 100, 50, 99)
    assert got.tolist() == [kernels.shuffle_source_row(i, 1365, 99) for i in range(100, 150)]


def test_thread_count_is_clamped():
    table = np.arange(7 * 13, dtype=np.uint8).reshape(7, 13)
    want = table[perm_of(7, 3)]
    for n_threads in (-5, 0, 1, 7, 8, 64, 65, 10 ** 6):
        assert np.array_equal(kernels.shuffle_gather_host(table, 0, 7, 3, n_threads=n_threads), want)


def test_range_beyond_the_table_is_an_invalid_argument():
    L = _lib.lib()
    table = np.zeros((10, 20), dtype=np.uint8)
    out = np.full((12, 20), 7, dtype=np.uint8)
    src, dst = ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    for first, n_out in ((0, 11), (5, 6), (10, 1), (11, 0), (2 ** 64 - 1, 2), (1, 2 ** 64 - 1)):
        assert L.bear_shuffle_gather_host(src, dst, 10, first, n_out, 20, 3, 4) == -1, (first, n_out)       # BEAR_ERR_INVALID_ARG
    assert (out == 7).all()                                                                               # nothing was written
    assert L.bear_shuffle_gather_host(src, dst, 10, 10, 0, 20, 3, 4) == 0
    assert L.bear_shuffle_gather_host(src, src, 10, 0, 10, 20, 3, 4) == -1                               # dst != src
    assert L.bear_shuffle_gather_host(None, dst, 10, 0, 10, 20, 3, 4) == -1
    with pytest.raises(_lib.BearError) as err:
        kernels.shuffle_gather_host(table, 5, 6, 3)
    assert err.value.status == -1 and "bear_shuffle_gather_host" in str(err.value)
    # the device entry refuses the same ranges before it touches a device (none is needed for the answer)
    assert L.bear_shuffle_rows_range(src, dst, 10, 5, 6, 20, 3, None) == -1
    assert L.bear_shuffle_rows_range(src, dst, 10, 10, 0, 20, 3, None) == 0
