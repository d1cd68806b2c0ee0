"""CPU tests of counting in passes over key ranges (bear_amd.summarize): the greedy cut of a bin histogram into ranges, and the
automatic choice between the single pass and passes as a pure function of the text's size, a pass's bytes and the free memory.
No test allocates near the 2^32 limit: these two functions, and the 64-bit positions of the two kernels, carry that part."""
import re

import numpy as np
import pytest

from util import HEADER

LIMIT = 2 ** 32 - 1


def check_cut(hist, max_pairs, ranges):
    hist = np.asarray(hist, dtype=np.uint64)
    covered = np.zeros(hist.size, dtype=int)
    end = 0
    for lo, hi, pairs in ranges:
        assert end <= lo < hi <= hist.size                               # ascending and disjoint
        end = hi
        assert hist[lo] > 0 and hist[hi - 1] > 0                         # empty stretches at either end belong to no range
        assert pairs == int(hist[lo:hi].sum())
        n_bins = int(np.count_nonzero(hist[lo:hi]))
        assert pairs <= max_pairs or n_bins == 1
        covered[lo:hi] += 1
        later = np.flatnonzero(hist[hi:])
        if later.size and pairs <= max_pairs:                            # greedy-maximal: the next non-empty bin would not have fitted
            assert pairs + int(hist[hi + later[0]]) > max_pairs
    assert np.all(covered[hist > 0] == 1)                                # every non-empty bin in exactly one range
    assert sum(p for _, _, p in ranges) == int(hist.sum())


def test_cut_ranges_by_hand():
    from bear_amd.summarize import cut_ranges
    hist = np.zeros(64, dtype=np.uint64)
    hist[[3, 4, 10, 11, 40]] = [5, 6, 30, 2, 7]
    assert cut_ranges(hist, 16) == [(3, 5, 11), (10, 11, 30), (11, 41, 9)]     # bin 10 is above the budget: a range of its own
    assert cut_ranges(hist, 50) == [(3, 41, 50)]
    assert cut_ranges(hist, 49) == [(3, 12, 43), (40, 41, 7)]
    assert cut_ranges(hist, 1) == [(b, b + 1, int(hist[b])) for b in (3, 4, 10, 11, 40)]
    assert cut_ranges(np.zeros(512, dtype=np.uint64), 16) == []
    assert cut_ranges(np.zeros(0, dtype=np.uint64), 16) == []
    one = np.zeros(8, dtype=np.uint64)
    one[7] = 3
    assert cut_ranges(one, 100) == [(7, 8, 3)]
    for m in (1, 5, 6, 7, 11, 16, 30, 43, 49, 50, 10 ** 12):
        check_cut(hist, m, cut_ranges(hist, m))


@pytest.mark.parametrize("seed", range(6))
def test_cut_ranges_on_random_histograms(seed):
    from bear_amd.summarize import cut_ranges
    rng = np.random.default_rng(seed)
    n_bins = int(rng.choice([8, 64, 512, 1 << 15]))
    hist = np.where(rng.random(n_bins) < rng.choice([0.02, 0.3, 1.0]), rng.integers(1, rng.choice([3, 200, 10 ** 6]), n_bins), 0).astype(np.uint64)
    hist[rng.integers(0, n_bins)] = 5000                                 # never empty, and one heavy bin
    for max_pairs in (1, 16, 4999, 5000, 10 ** 5, 10 ** 12):
        ranges = cut_ranges(hist, max_pairs)
        assert ranges
        check_cut(hist, max_pairs, ranges)


def test_a_bin_no_pass_can_index_is_named():
    from bear_amd.summarize import cut_ranges
    hist = np.zeros(1 << 18, dtype=np.uint64)
    hist[5] = 10
    hist[0] = LIMIT - 1                                                  # the most a pass indexes: attempted, as its own range
    assert cut_ranges(hist, 1000) == [(0, 1, LIMIT - 1), (5, 6, 10)]
    hist[0b011_010_001_000_000_000] = 2 ** 32                            # contexts ending in AAACGT (last letter in the top field)
    with pytest.raises(ValueError) as err:
        cut_ranges(hist, 1000)
    assert "AAACGT" in str(err.value)
    prot = np.zeros(1 << 15, dtype=np.uint64)
    prot[(19 << 10) | (20 << 5) | 0] = LIMIT                             # A[V: residue 0, the start symbol, residue 19
    with pytest.raises(ValueError) as err:
        cut_ranges(prot, 1000, alphabet="prot")
    assert "A[V" in str(err.value)


def test_bin_rule_constants_are_the_headers():
    from bear_amd import summarize
    src = open(HEADER).read()
    assert int(re.search(r"#define BEAR_COUNT_BIN_LETTERS (\d+)", src).group(1)) == summarize.BIN_LETTERS["dna"] == 6
    assert int(re.search(r"#define BEAR_COUNT_BIN_LETTERS_WIDE (\d+)", src).group(1)) == summarize.BIN_LETTERS["prot"] == 3
    assert [summarize.n_bins_of(lag) for lag in (1, 5, 6, 7, 21)] == [8, 1 << 15, 1 << 18, 1 << 18, 1 << 18]
    assert [summarize.n_bins_of(lag, "prot") for lag in (1, 3, 4, 12)] == [32, 1 << 15, 1 << 15, 1 << 15]


def test_automatic_decision():
    from bear_amd.summarize import cut_ranges, pass_plan
    per_pair = 30                                                         # about what a pass takes per pair
    # 5e9 positions go in passes however much memory is free, and no range exceeds 2^32 - 2 pairs
    n_pos = 5_000_000_000
    rng = np.random.default_rng(1)
    hist = rng.multinomial(n_pos - 10 ** 7, np.full(1 << 18, 2.0 ** -18)).astype(np.uint64)
    for free in (10 ** 9, 288 * 10 ** 9, 10 ** 15, 2 ** 62):
        max_pairs = pass_plan(n_pos, per_pair * (LIMIT - 1), free)
        assert max_pairs is not None and 1 <= max_pairs <= LIMIT - 1
        assert max_pairs * per_pair <= max(free // 2, per_pair)           # a pass stays within half of what is free
        ranges = cut_ranges(hist, max_pairs)
        assert len(ranges) >= 2 and all(p <= LIMIT - 1 for _, _, p in ranges)
        check_cut(hist, max_pairs, ranges)
    # the limit itself: 2^32 - 2 positions may take the single pass, 2^32 - 1 may not
    assert pass_plan(LIMIT - 1, per_pair * (LIMIT - 1), 2 ** 62) is None
    assert pass_plan(LIMIT, per_pair * (LIMIT - 1), 2 ** 62) == LIMIT - 1
    # a text that fits takes the single pass; one that needs more than half of the free memory does not
    assert pass_plan(10 ** 8, per_pair * 10 ** 8, 288 * 10 ** 9) is None
    assert pass_plan(10 ** 8, per_pair * 10 ** 8, 2 * per_pair * 10 ** 8) is None
    m = pass_plan(10 ** 8, per_pair * 10 ** 8, 2 * per_pair * 10 ** 8 - 2)
    assert m is not None and m < 10 ** 8 and m * per_pair <= per_pair * 10 ** 8 - 1
    assert pass_plan(10 ** 8, per_pair * 10 ** 8, 0) == 1                 # nothing free: the smallest passes, and the error is the device's
