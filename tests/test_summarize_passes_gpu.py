"""GPU tests of counting in passes over key ranges (bear_kmer_bin_hist + bear_kmer_sort_create_range, summarize.count_passes):
the table of the passes is the table of the single pass, row for row and count for count -- on the reference's example inputs
(also against the oracle's in-memory count), on protein sequences, on random sequences with invalid letters, and on a text
whose heaviest bin alone exceeds the budget; the entries at the ABI level against a host restatement of the key rule; the files
summarize writes; and a device-resident table in training.  Sizes are tiny on purpose: with max_pairs = 16 the 456 positions of
the example inputs already make a few dozen ranges per lag, some of them one oversize bin.  No test allocates near the 2^32
limit (tests/test_summarize_passes_cpu.py holds the decision function to it; both kernels index positions in 64 bits)."""
import ctypes
import os
import types

import numpy as np
import pytest

import bear_oracle as o
from conftest import GOLDEN
from test_prot_cpu import PROT

pytestmark = pytest.mark.gpu
SUM = os.path.join(GOLDEN, "summarize")
INVALID_ARG = -1


def _exdata_list(tmp_path):
    groups = [0, 0, 2, 1, 1]
    types_ = ["fa", "fq", "fq", "fa", "fq"]
    lst = tmp_path / "infiles.csv"
    lst.write_text("".join(f"{os.path.join(SUM, f'infile_{j}.{types_[j]}')},{groups[j]},{types_[j]}\n" for j in range(5)))
    return str(lst)


def _same_table(got, want, what):
    """(kmers, counts) pairs: equal as arrays, row order included."""
    assert got[0].shape == want[0].shape and got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0]), what
    assert got[1].shape == want[1].shape and got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), what


def _n_passes(text, grp, lag, n_groups, max_pairs, alphabet="dna"):
    """Pairs per range, as the passes meet them."""
    from bear_amd import summarize
    return [int(c.sum()) for _, c in summarize.count_passes(text, grp, lag, n_groups, max_pairs, alphabet=alphabet)]


@pytest.mark.parametrize("reverse", [False, True])
def test_example_inputs_dna(tmp_path, reverse):
    from bear_amd import summarize
    lst = _exdata_list(tmp_path)
    seqs, groups = summarize._load_sequences(lst)
    want = o.count_transitions(seqs, groups, 10, reverse=reverse)
    single = summarize.count_tables(lst, 10, reverse=reverse)
    text, grp, n_groups = summarize.load_text(lst, reverse)
    assert text.size == (456 if reverse else 228)
    for m in (16, 100):
        tables = summarize.count_tables(lst, 10, reverse=reverse, max_pairs=m)
        assert len(tables) == 10
        for li, (d, s) in enumerate(zip(tables, single)):
            _same_table((d.kmers, d.counts), (s.kmers, s.counts), (m, li + 1))
            got = {bytes(k).decode(): d.counts[:, i].astype(np.int64) for i, k in enumerate(d.kmers)}
            assert set(got) == set(want[li])
            for k in got:
                assert np.array_equal(got[k], want[li][k]), (m, li + 1, k)
    # the passes are real: many ranges at lag 10, and at lag 1 a bin above the budget that is counted as a range of its own
    assert len(_n_passes(text, grp, 10, n_groups, 16)) >= 12
    assert max(_n_passes(text, grp, 1, n_groups, 16)) > 16


def _protein_seqs(rng, n):
    seqs = ["".join(rng.choice(list(PROT), size=int(m))) for m in rng.integers(1, 40, size=n)]
    seqs[1] += "*"                                                  # an explicit stop
    seqs[2] = seqs[2][:3] + "X" + seqs[2][3:] + "MKV"               # a residue outside the 20
    return seqs + ["", "MK", "X"]


@pytest.mark.parametrize("lag", [1, 3, 5, 12])
def test_protein_sequences(lag):
    from bear_amd import summarize
    rng = np.random.default_rng(7)
    seqs = _protein_seqs(rng, 30)
    groups = [int(g) for g in rng.integers(0, 3, size=len(seqs))]
    text, grp = summarize.encode_sequences(seqs, groups, alphabet="prot")
    single = summarize.count_transitions(text, grp, lag, 3, alphabet="prot")
    assert single[0].shape[0] > 20 and single[1].shape[2] == 21
    _same_table(summarize.count_transitions(text, grp, lag, 3, alphabet="prot", max_pairs=16), single, lag)
    assert len(_n_passes(text, grp, lag, 3, 16, "prot")) >= 12


@pytest.mark.parametrize("lag", [1, 5, 13, 21])
def test_random_sequences_with_invalid_letters(lag):
    from bear_amd import summarize
    rng = np.random.default_rng(0)
    seqs = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(1, 400, size=300)]
    seqs += ["A", "", "ACGTNACGT", "NNNN"]                # shorter than the lag, empty, letters outside the alphabet
    seqs[5] = seqs[5] + "N" + seqs[6]
    groups = [int(g) for g in rng.integers(0, 4, size=len(seqs))]
    text, grp = summarize.encode_sequences(seqs, groups)
    assert 5e4 < text.size < 8e4
    single = summarize.count_transitions(text, grp, lag, 4)
    _same_table(summarize.count_transitions(text, grp, lag, 4, max_pairs=1000), single, lag)
    pieces = _n_passes(text, grp, lag, 4, 1000)
    assert sum(pieces) == int(single[1].sum()) and len(pieces) >= (5 if lag == 1 else 50)


def test_text_that_is_mostly_one_letter():
    """Poly-A reads with sparse other letters: the bin of the contexts ending in AAAAAA holds about half of all transitions."""
    from bear_amd import summarize
    rng = np.random.default_rng(4)
    seqs = ["".join(np.where(rng.random(200) < 0.9, "A", rng.choice(list("CGT"), size=200))) for _ in range(100)]
    groups = [i % 2 for i in range(len(seqs))]
    text, grp = summarize.encode_sequences(seqs, groups)
    assert text.size == 100 * 202 and (text == 0).mean() > 0.85
    lag, m = 8, 500
    single = summarize.count_transitions(text, grp, lag, 2)
    passes = summarize.count_transitions(text, grp, lag, 2, max_pairs=m)
    _same_table(passes, single, "poly-A")
    assert int(passes[1].sum()) == sum(len(s) + 1 for s in seqs)     # one per letter plus one stop per sequence
    pieces = _n_passes(text, grp, lag, 2, m)
    assert max(pieces) > 10 * m and len(pieces) > 10                 # one bin far above the budget, counted as its own range
    hist = _device_hist(text, lag, 5)
    assert int(hist[0]) == max(pieces)                               # bin 0: the last six letters are A


# ------------------------------------------------------------------------------------------------ the entries themselves
def host_keys(text, lag, bits, width):
    """The key rule restated on the host, on the code text as summarize.encode_sequences defines it (start marker `width`, stop
    and '[' `width - 1`, anything above the stop invalid): -> (key uint64 [n_pos], valid bool [n_pos])."""
    text = np.asarray(text).astype(np.int64)
    stop, start = width - 1, width
    pos = np.arange(text.size)
    key = np.zeros(text.size, dtype=np.uint64)
    started = np.zeros(text.size, dtype=bool)
    bad = np.zeros(text.size, dtype=bool)
    for i in range(1, lag + 1):                                       # letter lag - i of the context
        c = np.where(pos >= i, text[np.maximum(pos - i, 0)], start)
        c = np.where(started, stop, c)
        started |= c == start
        c = np.where(c == start, stop, c)
        bad |= c > stop
        key |= c.astype(np.uint64) << np.uint64(bits * (lag - i))
    return key, (text <= stop) & ~bad


def _device_hist(text, lag, width):
    import torch
    from bear_amd import _lib, summarize
    alphabet = "dna" if width == 5 else "prot"
    n_bins = summarize.n_bins_of(lag, alphabet)
    t = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    hist = torch.full((n_bins,), -1, dtype=torch.int64, device="cuda")          # (the entry zeroes it)
    _lib.call("bear_kmer_bin_hist", t.data_ptr(), t.numel(), lag, width, hist.data_ptr(), n_bins, None)
    torch.cuda.synchronize()
    return hist.cpu().numpy().view(np.uint64)


def _mixed_text(alphabet):
    from bear_amd import summarize
    rng = np.random.default_rng(12)
    if alphabet == "dna":
        seqs = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(1, 120, size=60)] + ["", "AC", "ACGNNACGTACGTTTT", "N"]
        seqs += ["A" * 300]                                           # more than one wave of equal neighbouring bins
    else:
        seqs = _protein_seqs(rng, 60) + ["W" * 200]
    groups = [int(g) for g in rng.integers(0, 3, size=len(seqs))]
    return summarize.encode_sequences(seqs, groups, alphabet=alphabet)


@pytest.mark.parametrize("alphabet,lags", [("dna", (1, 2, 6, 7, 13, 21)), ("prot", (1, 3, 4, 12))])
def test_histogram_against_the_host_key_rule(alphabet, lags):
    from bear_amd import summarize
    width, bits, letters = (5, 3, 6) if alphabet == "dna" else (21, 5, 3)
    text, grp = _mixed_text(alphabet)
    assert text.size > 1024                                           # several blocks of 256 positions, the last one partial
    assert text.size % 256 != 0
    for lag in lags:
        key, valid = host_keys(text, lag, bits, width)
        assert 0 < valid.sum() < text.size                            # some transitions are dropped
        n_bins = 1 << (bits * min(lag, letters))
        assert n_bins == summarize.n_bins_of(lag, alphabet)
        bins = (key[valid] >> np.uint64(bits * (lag - min(lag, letters)))).astype(np.int64)
        want = np.bincount(bins, minlength=n_bins).astype(np.uint64)
        got = _device_hist(text, lag, width)
        assert got.shape == want.shape and np.array_equal(got, want), lag
        kmers, counts = summarize.count_transitions(text, grp, lag, 3, alphabet=alphabet)
        assert int(got.sum()) == int(counts.sum()) == int(valid.sum())
        assert kmers.shape[0] == np.unique(key[valid]).size


@pytest.mark.parametrize("alphabet,lag", [("dna", 8), ("prot", 4)])
def test_create_range_entry(alphabet, lag):
    import torch
    from bear_amd import _lib, summarize
    width = 5 if alphabet == "dna" else 21
    L = _lib.lib()
    text, grp = _mixed_text(alphabet)
    t, g = torch.from_numpy(text).cuda(), torch.from_numpy(grp).cuda()
    hist = _device_hist(text, lag, width)
    n_bins = hist.size
    single = summarize.count_transitions(text, grp, lag, 3, alphabet=alphabet)

    def create(lo, hi, capacity, lag_=lag, width_=width):
        h, n_rows = ctypes.c_void_p(12345), ctypes.c_uint64(7)
        st = L.bear_kmer_sort_create_range(t.data_ptr(), g.data_ptr(), t.numel(), lag_, width_, lo, hi, capacity, ctypes.byref(h),
                                           ctypes.byref(n_rows), None)
        return st, h, n_rows.value

    def rows_of(h, n):
        try:
            km = torch.zeros((n, lag), dtype=torch.uint8, device="cuda")
            cn = torch.zeros((3, n, width), dtype=torch.int32, device="cuda")
            assert L.bear_kmer_sort_reduce(h, 3, km.data_ptr(), None, cn.data_ptr(), None) == 0
            torch.cuda.synchronize()
        finally:
            L.bear_kmer_sort_destroy(h)
        return km.cpu().numpy(), cn.cpu().numpy().view(np.uint32)

    ranges = summarize.cut_ranges(hist, 100, alphabet)
    assert len(ranges) >= 8
    total, first = 0, None
    for lo, hi, pairs in ranges:
        st, h, n = create(lo, hi, pairs)
        assert st == 0 and h.value
        piece = rows_of(h, n)
        _same_table(piece, (single[0][total:total + n], single[1][:, total:total + n]), (lo, hi))
        first = first or (lo, hi, pairs, piece)
        total += n
    assert total == single[0].shape[0]                                # the ranges' rows are the single pass's rows
    # a capacity that is not the range's number of pairs: refused, no handle, nothing overrun -- and the next call is served
    lo, hi, pairs, piece = first
    for wrong in (pairs - 1, pairs + 1, 0):
        st, h, n = create(lo, hi, wrong)
        assert st == INVALID_ARG and h.value is None and n == 0, wrong
    st, h, n = create(lo, hi, pairs)
    assert st == 0
    _same_table(rows_of(h, n), piece, "after a refused call")
    # a whole-key-space range with the histogram's sum is the single pass
    st, h, n = create(0, n_bins, int(hist.sum()))
    assert st == 0 and n == single[0].shape[0]
    _same_table(rows_of(h, n), single, "one range")
    # a range without transitions, capacity 0: an empty handle
    empty = int(np.flatnonzero(hist == 0)[0])
    st, h, n = create(empty, empty + 1, 0)
    assert st == 0 and n == 0
    L.bear_kmer_sort_destroy(h)
    # arguments
    for bad in (dict(lo=0, hi=n_bins + 1, capacity=10), dict(lo=3, hi=3, capacity=10), dict(lo=0, hi=1, capacity=10, width_=7),
                dict(lo=0, hi=1, capacity=10, lag_=13, width_=21), dict(lo=0, hi=1, capacity=10, lag_=22, width_=5),
                dict(lo=0, hi=1, capacity=2 ** 32 - 1)):
        st, h, n = create(**bad)
        assert st == INVALID_ARG and h.value is None and n == 0, bad
    hist_dev = torch.zeros(n_bins, dtype=torch.int64, device="cuda")
    assert L.bear_kmer_bin_hist(t.data_ptr(), t.numel(), lag, width, hist_dev.data_ptr(), n_bins - 1, None) == INVALID_ARG
    assert L.bear_kmer_bin_hist(t.data_ptr(), t.numel(), lag, 7, hist_dev.data_ptr(), n_bins, None) == INVALID_ARG
    assert L.bear_kmer_bin_hist(t.data_ptr(), t.numel(), 13, 21, hist_dev.data_ptr(), 1 << 15, None) == INVALID_ARG


def test_pass_bytes():
    from bear_amd import _lib
    L = _lib.lib()

    def bytes_of(n, lag, width):
        b = ctypes.c_uint64(7)
        st = L.bear_kmer_sort_bytes(n, lag, width, ctypes.byref(b))
        return st, b.value
    for lag, width in ((1, 5), (13, 5), (21, 5), (3, 21), (12, 21)):
        sizes = [0, 1, 1000, 10 ** 6, 10 ** 8, 2 ** 32 - 2]
        got = [bytes_of(n, lag, width) for n in sizes]
        assert all(st == 0 for st, _ in got)
        b = [v for _, v in got]
        assert b[0] == 0 and all(x <= y for x, y in zip(b, b[1:]))     # monotone
        assert all(v >= 24 * n for n, v in zip(sizes, b))              # the two key and the two value buffers at least
        assert b[4] < 64 * sizes[4]                                    # and no more than a few such buffers
    assert bytes_of(2 ** 32 - 1, 5, 5)[0] == INVALID_ARG
    assert bytes_of(100, 5, 7)[0] == INVALID_ARG and bytes_of(100, 13, 21)[0] == INVALID_ARG and bytes_of(100, 0, 5)[0] == INVALID_ARG


# ------------------------------------------------------------------------------------------------ files, training
def test_files_are_byte_identical(tmp_path, monkeypatch):
    from bear_amd import summarize
    lst = _exdata_list(tmp_path)
    calls = []
    real = summarize.count_passes
    monkeypatch.setattr(summarize, "count_passes", lambda *a, **k: calls.append(a[4]) or real(*a, **k))
    out = {}
    for name in ("single", "passes"):
        if name == "passes":
            monkeypatch.setenv("BEAR_AMD_COUNT_MAX_PAIRS", "16")
        else:
            monkeypatch.delenv("BEAR_AMD_COUNT_MAX_PAIRS", raising=False)
        (tmp_path / name).mkdir()
        args = types.SimpleNamespace(file=lst, out_prefix=str(tmp_path / name / "out"), l=10, nf=False, r=True, mf=1e-6)
        out[name] = summarize.main(args)
        if name == "single":
            assert calls == []
    assert calls == [16] * 20                                          # ten lags, forward and with reverse complements
    assert out["single"] == out["passes"] and out["single"][0] > 1 and out["single"][1] > 1
    files = sorted(os.listdir(tmp_path / "single"))
    assert files == sorted(os.listdir(tmp_path / "passes"))
    assert len(files) == 10 * (out["single"][0] + out["single"][1]) and any("_rev_" in f for f in files)
    for f in files:
        assert (tmp_path / "single" / f).read_bytes() == (tmp_path / "passes" / f).read_bytes(), f


def test_device_resident_tables_from_passes_train_like_host_tables(tmp_path):
    import torch
    from bear_amd import ar_funcs, bear_net, summarize
    rng = np.random.default_rng(5)
    fa = tmp_path / "s.fa"
    fa.write_text("".join(f">s{i}\n{''.join(rng.choice(list('ACGT'), size=int(n)))}\n" for i, n in enumerate(rng.integers(10, 60, size=200))))
    lst = tmp_path / "l.csv"
    lst.write_text(f"{fa},0,fa\n")
    host = summarize.count_tables(str(lst), 5)
    dev = summarize.count_tables(str(lst), 5, on_device=True, max_pairs=64)
    for h, d in zip(host, dev):
        assert d.kmers_dev.is_cuda and d.counts_dev.is_cuda and d.num_rows == h.num_rows
        _same_table((d.kmers, d.counts), (h.kmers, h.counts), h.num_rows)
    losses = []
    for data in (host[4], dev[4]):
        torch.manual_seed(0)
        ls = []
        bear_net.train(data.repeat(2), data.num_rows, 2, 0, "dna", 5, ar_funcs.make_ar_func_linear, {}, 0.01, "Adam", False, loss_save=ls)
        losses.append(ls)
    assert len(losses[0]) == 2 and np.all(np.isfinite(losses[0]))
    assert np.allclose(losses[0], losses[1], rtol=1e-13)
