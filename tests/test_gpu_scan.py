"""The exclusive prefix sums every on-GPU output stage takes (mapper_amd/csrc/xm_scan.h), alone through xm_test_scan, against numpy.cumsum for exact
equality: the thread (16), gather-block (256) and scan-block (4096) edges, two blocks plus one item and sixteen blocks plus one, with one, two and three
lengths an item; block sums beyond 32 bits; the compaction form over a mask; and the block-sum buffer used again by a smaller scan."""
import ctypes as C

import numpy as np
import pytest

from mapper_amd import _capi

SIZES = [0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8193, 256 * 256 + 1]
GUARD = -7


def device_scan(lens, keep=None):
    """lens: int64 [channels, n]; keep: None or n bytes of 0 / 1 -> (offsets [channels, n + 1], kept indices or None).  Nothing is written behind the arrays."""
    L = _capi.lib()
    lens = np.ascontiguousarray(lens, np.int64)
    channels, n = lens.shape
    off = np.full(channels * (n + 1) + 1, GUARD, np.int64)
    kept = np.full(n + 1, GUARD, np.int64)
    count = C.c_int64(GUARD)
    mask = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    if L.xm_test_scan(0, channels, n, lens.ctypes.data, None if mask is None else mask.ctypes.data, off.ctypes.data, kept.ctypes.data, C.byref(count)):
        raise RuntimeError(L.xm_last_error().decode())
    assert off[-1] == GUARD
    if mask is None:
        assert count.value == GUARD and np.all(kept == GUARD)
        return off[:-1].reshape(channels, n + 1), None
    assert 0 <= count.value <= n and np.all(kept[count.value:] == GUARD)
    return off[:-1].reshape(channels, n + 1), kept[:count.value].copy()


def want_offsets(lens):
    """numpy.cumsum with the 0 in front: [channels, n + 1]."""
    lens = np.asarray(lens, np.int64)
    return np.concatenate([np.zeros((lens.shape[0], 1), np.int64), np.cumsum(lens, axis=1, dtype=np.int64)], axis=1)


def values(kind, channels, n, seed):
    if kind == "zero":
        return np.zeros((channels, n), np.int64)
    if kind == "one":
        return np.ones((channels, n), np.int64)
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1001, (channels, n), dtype=np.int64)
    v[rng.random((channels, n)) < 1 / 3] = 0
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_offsets_equal_cumsum(n, channels):
    for kind in ("zero", "one", "random"):
        lens = values(kind, channels, n, seed=1000 * channels + n)
        got, _ = device_scan(lens)
        assert np.array_equal(got, want_offsets(lens)), kind
    if n >= 255:
        assert (lens == 0).sum() > lens.size // 4 and len({tuple(row) for row in lens}) == channels   # zeros among the lengths, and no two channels alike


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_block_sums_beyond_32_bits(channels):
    """4097 items of up to 2^31 - 1: the first block's sum is far beyond 2^32, so any 32-bit narrowing of a thread's, a block's or the running sum shows."""
    rng = np.random.default_rng(77 + channels)
    lens = rng.integers(0, 2**31, (channels, 4097), dtype=np.int64)
    lens[:, 0] = lens[:, 4095] = lens[:, 4096] = 2**31 - 1
    got, _ = device_scan(lens)
    want = want_offsets(lens)
    assert np.array_equal(got, want) and want[:, 16].min() > 2**32 and want[:, -1].min() > 2**40


def masks(n):
    none, every = np.zeros(n, np.uint8), np.ones(n, np.uint8)
    seventeenth = np.zeros(n, np.uint8)
    seventeenth[::17] = 1
    only = np.zeros(n, np.uint8)
    if n > 4096:
        only[4096] = 1
    return [("none", none), ("all", every), ("every 17th", seventeenth), ("item 4096", only)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_compaction_lists_the_kept_items_in_order(n):
    lens = values("random", 2, n, seed=n)
    want = want_offsets(lens)
    for name, mask in masks(n):
        got, kept = device_scan(lens, mask)
        assert np.array_equal(got, want), name
        assert np.array_equal(kept, np.flatnonzero(mask)), name


@pytest.mark.gpu
def test_block_sums_are_reused_by_a_smaller_scan():
    """The entry keeps its buffers from call to call, as every stage keeps its block sums: three blocks' worth first, then one item."""
    big, small = values("random", 3, 8193, seed=5), np.array([[5], [0], [9]], np.int64)
    got, kept = device_scan(big, np.ones(8193, np.uint8))
    assert np.array_equal(got, want_offsets(big)) and np.array_equal(kept, np.arange(8193))
    got, kept = device_scan(small, np.ones(1, np.uint8))
    assert np.array_equal(got, want_offsets(small)) and np.array_equal(kept, [0])
    got, kept = device_scan(big[:1], np.zeros(8193, np.uint8))
    assert np.array_equal(got, want_offsets(big[:1])) and len(kept) == 0
