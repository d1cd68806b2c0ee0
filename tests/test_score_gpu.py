"""GPU tests of scoring on the device (kernels_score.h, get_var_probs.DeviceCounter): the three kernels against plain Python /
NumPy, the counter against make_sequence_counter, and get_bear_probs / get_bear_probs_seqs with a DeviceCounter against the host
``counter=`` path of the same call (same seed, so the same sampled table: the scores differ by summation order only)."""
import configparser
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bear_amd import core, get_var_probs, kernels
from conftest import ROOT
from test_prot_cpu import PROT, write_prot_tsv

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
VANS = np.array([0.1, 1.0, 10.0])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _codes(strings, alphabet_name):
    lut = get_var_probs._symbol_lut(alphabet_name)
    text = lut[np.frombuffer("".join(strings).encode(), dtype=np.uint8)]
    seg = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    return text, seg


def _key(kmer, alphabet_name):
    """The key restated from the strings: position of each character among the alphabet's characters and '[' in byte order."""
    letters = sorted([str(c) for c in core.alphabets_en[alphabet_name][:-1]] + ["["])
    bits = 3 if len(letters) == 5 else 5
    key = 0
    for ch in kmer:
        key = (key << bits) | letters.index(ch)
    return key


# ------------------------------------------------------------------------------------------- 1. kmer_find
@pytest.mark.parametrize("n_table", [0, 1, 2, 1000])
@pytest.mark.parametrize("span", ["dna21", "prot12"])
def test_kmer_find_against_a_dict(n_table, span):
    rng = np.random.default_rng(n_table + len(span))
    lo, hi = (2 ** 62, 2 ** 63 - 2) if span == "dna21" else (5, 21 * 32 ** 11)       # dna lag 21: bit 62 set; prot lag 12: 60 bits
    table = np.unique(rng.integers(lo + 10, hi - 10, size=n_table, dtype=np.int64))
    while table.size < n_table:
        table = np.unique(np.concatenate([table, rng.integers(lo + 10, hi - 10, size=n_table, dtype=np.int64)]))[:n_table]
    index = {int(k): i for i, k in enumerate(table)}
    present = rng.choice(table, size=min(300, 3 * n_table)) if n_table else np.zeros(0, dtype=np.int64)      # duplicated queries
    between = rng.integers(lo + 10, hi - 10, size=300, dtype=np.int64)
    edges = np.array([lo, lo + 9, hi - 9, hi, 0, 2 ** 63 - 1], dtype=np.int64)                               # below the minimum, above the maximum
    near = np.concatenate([table[:50] - 1, table[:50] + 1, table[-50:] + 1]) if n_table else np.zeros(0, dtype=np.int64)
    query = np.concatenate([present, between, edges, near, present])
    for q in (query, np.sort(query)):
        want = np.array([index.get(int(x), -1) for x in q], dtype=np.int32)
        got = kernels.kmer_find(_dev(table), _dev(q))
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
        assert (want >= 0).sum() >= 2 * present.size and (want < 0).sum() >= 300
    none = kernels.kmer_find(_dev(table), torch.empty(0, dtype=torch.int64, device="cuda"))
    assert none.shape == (0,) and none.dtype == torch.int32


# ------------------------------------------------------------------------------------------- 2. score_transitions
@pytest.mark.parametrize("alphabet_name,lag", [("dna", 1), ("dna", 21), ("prot", 12), ("rna", 4)])
def test_score_transitions_against_python_slicing(alphabet_name, lag):
    rng = np.random.default_rng(lag)
    letters = [str(c) for c in core.alphabets_en[alphabet_name][:-1]]

    def rand(n):
        return "".join(rng.choice(letters, n))
    strings = ["[" * lag + rand(40) + "]",              # contexts holding '[', a next symbol ']'
               rand(lag - 1), rand(lag), rand(lag + 1),  # shorter than lag, exactly lag (no transition), one transition
               "", "[" * lag + "]", "[" * (lag - 1) + rand(3) + "]", rand(300), "[" * lag + rand(700) + "]", ""]
    text, seg = _codes(strings, alphabet_name)
    W = len(letters) + 1
    keys, got_letters = kernels.score_transitions(_dev(text), _dev(seg), lag, kernels.score_ranks(alphabet_name))
    keys, got_letters = keys.cpu().numpy(), got_letters.cpu().numpy()
    assert keys.dtype == np.int64 and got_letters.dtype == np.uint8 and keys.shape == got_letters.shape == text.shape
    index = {ch: i for i, ch in enumerate(letters + ["]"])}
    n_trans = 0
    for s, a in zip(strings, seg[:-1]):
        for p in range(len(s)):
            if p < lag:
                assert keys[a + p] == -1 and got_letters[a + p] == 0xFF, (s, p)
            else:
                assert keys[a + p] == _key(s[p - lag:p], alphabet_name) and got_letters[a + p] == index[s[p]], (s, p)
                n_trans += 1
    assert n_trans == sum(max(0, len(s) - lag) for s in strings) > 1000
    assert int(got_letters.max(initial=0, where=got_letters != 0xFF)) == W - 1
    # distinct keys ascending = the k-mer strings sorted
    kmers = sorted({s[p - lag:p] for s in strings for p in range(lag, len(s))})
    assert np.array_equal(np.unique(keys[keys >= 0]), np.array([_key(k, alphabet_name) for k in kmers], dtype=np.int64))


# ------------------------------------------------------------------------------------------- 3. score_sum
SUM_LENS = [7, 0, 70_000, 1, kernels.SCORE_CHUNK, kernels.SCORE_CHUNK + 1, 0, 3]       # 70 000 crosses the chunking; its threshold


@pytest.fixture(scope="module")
def sum_case():
    rng = np.random.default_rng(11)
    n_t = sum(SUM_LENS)
    rows = rng.integers(0, 37, size=n_t).astype(np.int32)
    unit = rng.random(n_t)
    skip = rng.random(n_t) < 0.1
    rows[rng.random(n_t) < 0.01] = -1
    seg = np.concatenate([[0], np.cumsum(SUM_LENS)]).astype(np.int64)
    return rows, unit, skip, seg


@pytest.mark.parametrize("W", [5, 21])
@pytest.mark.parametrize("M,S", [(1, 1), (3, 41), (4, 64), (2, 100)])
def test_score_sum_against_a_sequential_sum(sum_case, W, M, S):
    rows, unit, skip, seg = sum_case
    K = 37
    rng = np.random.default_rng(W * 1000 + M * S)
    lp = -rng.exponential(3.0, size=(K, W, M, S))
    letters = np.where(skip, 0xFF, (unit * W).astype(np.int64)).astype(np.uint8)
    args = (_dev(lp), _dev(rows), _dev(letters), _dev(seg))
    got = kernels.score_sum(*args)
    assert got.shape == (len(SUM_LENS), M, S) and got.dtype == torch.float64
    again = kernels.score_sum(*args)
    assert torch.equal(got, again)                                     # the same call twice: equal bits
    got = got.cpu().numpy()
    live = (letters != 0xFF) & (rows >= 0)
    for i, n in enumerate(SUM_LENS):
        sl = slice(seg[i], seg[i + 1])
        terms = lp[rows[sl][live[sl]], letters[sl][live[sl]]]          # [n live, M, S] in text order
        want = np.zeros((M, S))
        for x in terms:
            want += x
        mass = np.abs(terms).sum(0)
        err = np.abs(got[i] - want)
        assert np.all(err <= (n + 2) * U * mass), (i, n, float((err / np.maximum(mass, 1e-300)).max() / U))
        if n <= kernels.SCORE_CHUNK:
            assert np.array_equal(got[i], want)                        # a short segment is this very sum, front to back
    # a segment's sum does not depend on where it stands in the text: the long one moved to the front
    order = [2, 0, 1, 3, 4, 5, 6, 7]
    idx = np.concatenate([np.arange(seg[i], seg[i + 1]) for i in order])
    seg2 = np.concatenate([[0], np.cumsum([SUM_LENS[i] for i in order])]).astype(np.int64)
    moved = kernels.score_sum(_dev(lp), _dev(rows[idx]), _dev(letters[idx]), _dev(seg2)).cpu().numpy()
    assert np.array_equal(moved, got[order])


LONG_LENS = [5, 2049, 4097, 0, 2049, 1]      # starts 0, 5, 2054, 6151, 6151, 8200: text block 1 (positions 2048 .. 4095) holds the
#                                              second chunk of segment 1 (slot 2 g) AND chunk 0 of segment 2 (slot 2 g + 1); segment 4
#                                              starts directly behind an empty one


@pytest.mark.parametrize("W", [5, 21])
@pytest.mark.parametrize("M,S", [(1, 1), (2, 33)])
def test_score_sum_of_long_segments_bit_for_bit(W, M, S):
    """The order of a long segment's sum is fully specified: every chunk of SCORE_CHUNK transitions front to back from 0.0, then the
    chunks' sums in order from 0.0, plain fp64 adds.  A NumPy sum in that order equals the device bytes, wherever the segment stands."""
    assert kernels.SCORE_CHUNK == 2048
    K = 37
    rng = np.random.default_rng(W * 1000 + M * S)
    n_t = sum(LONG_LENS)
    rows = rng.integers(0, K, size=n_t).astype(np.int32)
    rows[rng.random(n_t) < 0.01] = -1
    letters = np.where(rng.random(n_t) < 0.1, 0xFF, (rng.random(n_t) * W).astype(np.int64)).astype(np.uint8)
    lp = -rng.exponential(3.0, size=(K, W, M, S))
    seg = np.concatenate([[0], np.cumsum(LONG_LENS)]).astype(np.int64)
    assert seg.tolist() == [0, 5, 2054, 6151, 6151, 8200, 8201]

    def chunk_sum(a, b):
        acc = np.zeros((M, S))
        for t in range(a, b):
            if letters[t] != 0xFF and rows[t] >= 0:
                acc = acc + lp[rows[t], letters[t]]
        return acc
    want = []
    for a, b in zip(seg[:-1], seg[1:]):
        if b - a <= kernels.SCORE_CHUNK:
            want.append(chunk_sum(a, b))
        else:
            acc = np.zeros((M, S))
            for c in range(a, b, kernels.SCORE_CHUNK):
                acc = acc + chunk_sum(c, min(c + kernels.SCORE_CHUNK, b))
            want.append(acc)
    got = kernels.score_sum(_dev(lp), _dev(rows), _dev(letters), _dev(seg)).cpu().numpy()
    for i in range(len(LONG_LENS)):
        assert np.array_equal(got[i], want[i]), (i, LONG_LENS[i], float(np.abs(got[i] - want[i]).max()))
    for order in ([2, 4, 1, 0, 5, 3], [5, 4, 3, 2, 1, 0]):
        idx = np.concatenate([np.arange(seg[i], seg[i + 1]) for i in order])
        seg2 = np.concatenate([[0], np.cumsum([LONG_LENS[i] for i in order])]).astype(np.int64)
        moved = kernels.score_sum(_dev(lp), _dev(rows[idx]), _dev(letters[idx]), _dev(seg2)).cpu().numpy()
        for j, i in enumerate(order):
            assert np.array_equal(moved[j], want[i]), (order, i)


def test_score_sum_edges():
    lp = _dev(-np.ones((3, 5, 2, 2)))
    none = torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.uint8, device="cuda")
    out = kernels.score_sum(lp, *none, _dev(np.zeros(4, dtype=np.int64)))
    assert out.shape == (3, 2, 2) and not out.any()
    assert kernels.score_sum(lp, *none, _dev(np.zeros(1, dtype=np.int64))).shape == (0, 2, 2)
    with pytest.raises(ValueError):
        kernels.score_sum(lp, _dev(np.zeros(3, dtype=np.int32)), _dev(np.zeros(2, dtype=np.uint8)), _dev(np.array([0, 3])))


def test_get_pdf_leaves_the_table_on_the_device():
    kmers = np.array(sorted(["ACG", "[[A", "TTT", "GAT"]))
    counts = np.arange(4 * 5, dtype=np.float64).reshape(4, 1, 5)
    for get_map in (True, False):
        on_host = get_var_probs.get_pdf(kmers, counts, None, None, 6, VANS, 0, "dna", get_map, output="numpy", seed=4)
        on_dev = get_var_probs.get_pdf(kmers, counts, None, None, 6, VANS, 0, "dna", get_map, output="device", seed=4)
        assert on_dev.is_cuda and on_dev.shape == (4, 5, 3, 1 if get_map else 6) and np.array_equal(on_dev.cpu().numpy(), on_host)


# ------------------------------------------------------------------------------------------- 4. the counter, called
DNA_SEQS = ["ACGTTGCAAGTCAT", "TTTACATATTACA", "ATATAGATACATTTAG", "ACA", "GATTACA", "T", "ATATTACATTAGATACATATTAGACATTACATAG"]
PROT_SEQS = ["MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQ", "MKTAYIAKQRWISFVKSHFSRQ", "KKKKKKKKAKKKKKKK", "ACDEFGHIKLMNPQRSTVWY", "MK"]


def _queries(seqs, lag, alphabet_name, rng):
    letters = [str(c) for c in core.alphabets_en[alphabet_name][:-1]]
    q = set()
    for s in seqs:
        p = "[" * lag + s + "]"
        q.update(p[j:j + lag] for j in range(len(p) - lag))
    q = sorted(q) + ["".join(rng.choice(letters, lag)) for _ in range(40)] + ["[" * lag, letters[1] * lag, "N" * lag, "x", ""]
    return q + q[:5]


@pytest.mark.parametrize("alphabet_name,lag,reverse", [("dna", 3, True), ("dna", 3, False), ("dna", 21, True), ("prot", 4, False),
                                                       ("prot", 12, False)])
@pytest.mark.parametrize("no_end", [False, True])
def test_device_counter_equals_sequence_counter(alphabet_name, lag, reverse, no_end):
    seqs = DNA_SEQS if alphabet_name == "dna" else PROT_SEQS
    host = get_var_probs.make_sequence_counter(seqs, lag, reverse=reverse, no_end=no_end, alphabet_name=alphabet_name)
    dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=reverse, no_end=no_end, alphabet_name=alphabet_name)
    assert dev.kmers.is_cuda and dev.counts.is_cuda and dev.keys.is_cuda and dev.lag == lag
    assert dev.kmers.shape == (dev.counts.shape[0], lag) and dev.counts.shape[1] == dev.width == len(core.alphabets_en[alphabet_name])
    assert bool((dev.keys[1:] > dev.keys[:-1]).all()) and dev.keys.numel() == dev.kmers.shape[0]
    q = _queries(seqs, lag, alphabet_name, np.random.default_rng(lag))
    want, got = host(q), dev(q)
    assert got.shape == want.shape == (len(q), dev.width) and got.dtype == want.dtype
    assert np.array_equal(got, want) and want.sum() > 0 and (want.sum(1) == 0).any()
    q2 = np.array(q[:6]).reshape(2, 3)
    assert np.array_equal(dev(q2), host(q2)) and dev(q2).shape == (2, 3, dev.width)
    assert dev([]).shape == host([]).shape


def test_device_counter_from_a_device_dataset():
    """from_dataset on a DeviceCountDataset (two groups counted on the device): column 1 in place, equal to the host counter of
    that group's sequences; a shuffled table is looked up all the same (the keys are sorted once, whatever the row order)."""
    from bear_amd import dataloader, summarize
    groups = [0, 1, 1, 0, 1, 0, 1]
    text, grp = summarize.encode_sequences(DNA_SEQS, groups, reverse=False)
    kmers, counts = summarize.count_transitions(text, grp, 3, 2, on_device=True)
    data = dataloader.DeviceCountDataset(kmers, counts, "dna", 100)
    host = get_var_probs.make_sequence_counter([s for s, g in zip(DNA_SEQS, groups) if g == 1], 3, reverse=False)
    q = _queries(DNA_SEQS, 3, "dna", np.random.default_rng(0))
    dev = get_var_probs.DeviceCounter.from_dataset(data, 1)
    assert dev.counts.data_ptr() == counts[1].data_ptr() and np.array_equal(dev(q), host(q))
    perm = torch.randperm(kmers.shape[0], device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    shuffled = dataloader.DeviceCountDataset(kmers[perm], counts[:, perm], "dna", 100)
    assert np.array_equal(get_var_probs.DeviceCounter.from_dataset(shuffled, 1)(q), host(q))
    with pytest.raises(ValueError, match="twice"):
        get_var_probs.DeviceCounter(torch.cat([kmers, kmers[:1]]), torch.cat([counts[1], counts[1, :1]]), "dna")


# ------------------------------------------------------------------------------------------- 5. / 6. whole calls
def _table_of(kmers, counter, ar_func, h, alphabet_name, get_map, mc, seed):
    """The sampled table of the sorted distinct k-mers of a call, as the host counter= path draws it -> ({k-mer: row}, |lp| [K, W, M, S])."""
    lp = get_var_probs.get_pdf(kmers, counter(kmers)[:, None, :], h, ar_func, mc, VANS, 0, alphabet_name, get_map, output="numpy",
                               seed=seed, row_base=0)
    return {k: i for i, k in enumerate(kmers)}, np.abs(lp)


def _mass(strings, lag, index, lp_abs, alphabet_name):
    """(transitions, sum_t |lp_t| [M, S]) over the windows / sequences given."""
    letter = {str(b): j for j, b in enumerate(core.alphabets_en[alphabet_name])}
    n, mass = 0, np.zeros(lp_abs.shape[2:])
    for s in strings:
        for p in range(lag, len(s)):
            mass += lp_abs[index[s[p - lag:p]], letter[s[p]]]
            n += 1
    return n, mass


def _var_windows(wt, var, lag):
    wt_aa, mt_aa, pos = get_var_probs.parse_var(var)
    padded = "[" * lag + wt + "]"
    pos += lag
    return [padded[pos - lag:pos] + mt_aa + padded[pos + len(wt_aa):pos + lag + len(wt_aa)], padded[pos - lag:pos + lag + len(wt_aa)]]


def _check_vars(got, want, wt, vars_, lag, index, lp_abs, alphabet_name):
    assert got.shape == want.shape and np.isfinite(got).all()
    for i, v in enumerate(vars_):
        n, mass = _mass(_var_windows(wt, v, lag), lag, index, lp_abs, alphabet_name)
        err = np.abs(got[i] - want[i]).reshape(mass.shape)
        assert np.all(err <= (n + 2) * U * mass), (v, n, float((err / mass).max() / U))


DNA_WT = "ACGTTGCAAGTC"
DNA_VARS = ["A0T", "C11A", "GTT2A", "T4TGGGG", "G5", "C11", "AC0", "C1GG", "TC10A", "A8T"]
PROT_WT = PROT_SEQS[0]
PROT_VARS = ["M0A", "Q32Y", "K1W", "TAY2W", "AY3", "T2TGW", "A6", "5R", "L28P", "Q32", "V31VVV", "I5WWWWW"]
VAR_CASES = {"dna": (3, DNA_WT, DNA_VARS, DNA_SEQS, True), "prot": (4, PROT_WT, PROT_VARS, PROT_SEQS, False)}


def _var_call(alphabet_name, counter, get_map, vars_=None, seed=5):
    lag, wt, default_vars, _, _ = VAR_CASES[alphabet_name]
    return get_var_probs.get_bear_probs(None, wt, default_vars if vars_ is None else vars_, 0, mc_samples=7, vans=VANS, get_map=get_map,
                                        lag=lag, alphabet_name=alphabet_name, seed=seed, counter=counter)


@pytest.mark.parametrize("alphabet_name", ["dna", "prot"])
@pytest.mark.parametrize("get_map", [True, False])
def test_get_bear_probs_on_the_device(alphabet_name, get_map):
    lag, wt, vars_, seqs, reverse = VAR_CASES[alphabet_name]
    host = get_var_probs.make_sequence_counter(seqs, lag, reverse=reverse, alphabet_name=alphabet_name)
    dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=reverse, alphabet_name=alphabet_name)
    parsed = [get_var_probs.parse_var(v) for v in vars_]
    kmers = get_var_probs._get_all_kmers_vars(parsed, "[" * lag + wt + "]", lag)
    assert (host(kmers).sum(1) == 0).any()                                     # a window holds a k-mer the counter never saw
    assert any(p == 0 for _, _, p in parsed) and any(p + len(a) == len(wt) for a, _, p in parsed)      # first and last position
    assert any(len(a) > 1 for a, _, _ in parsed) and any(not m for _, m, _ in parsed) and any(len(m) > len(a) for a, m, _ in parsed)
    want = _var_call(alphabet_name, host, get_map)
    got = _var_call(alphabet_name, dev, get_map)
    assert got.shape == ((len(vars_), 3) if get_map else (len(vars_), 3, 7))
    index, lp_abs = _table_of(kmers, host, None, None, alphabet_name, get_map, 7, 5)
    _check_vars(got, want, wt, vars_, lag, index, lp_abs, alphabet_name)
    assert np.abs(want).max() > 0.1
    empty = _var_call(alphabet_name, dev, get_map, vars_=[])
    assert empty.shape == ((0, 3) if get_map else (0, 3, 7))
    if not get_map:      # seed=None takes one seed from numpy's global generator, as the host path does
        np.random.seed(3)
        a = _var_call(alphabet_name, host, False, seed=None)
        state = np.random.get_state()[1].copy()
        np.random.seed(3)
        b = _var_call(alphabet_name, dev, False, seed=None)
        assert np.array_equal(np.random.get_state()[1], state) and np.allclose(a, b, rtol=1e-12, atol=1e-12)
        assert not np.allclose(a, want)


SEQ_CASES = {"dna": (3, ["ACGTTGCAAGTC", "ACACACACACACACAC", "TTT", "GGGCCCGGG", "A" * 40 + "C"], DNA_SEQS, True),
             "prot": (4, [PROT_WT, "KKKKKKKKKKAKKKKKKKKKK", "MKTA", "WWWWWWCW", PROT_SEQS[3]], PROT_SEQS, False)}


@pytest.mark.parametrize("alphabet_name", ["dna", "prot"])
@pytest.mark.parametrize("no_ends", [False, True])
def test_get_bear_probs_seqs_on_the_device(alphabet_name, no_ends):
    lag, queries, seqs, reverse = SEQ_CASES[alphabet_name]
    assert any(len(s) == lag for s in queries)
    host = get_var_probs.make_sequence_counter(seqs, lag, reverse=reverse, no_end=no_ends, alphabet_name=alphabet_name)
    dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=reverse, no_end=no_ends, alphabet_name=alphabet_name)
    strings = queries if no_ends else ["[" * lag + s + "]" for s in queries]
    kmers = get_var_probs._get_all_kmers_seqs(strings, lag)
    assert (host(kmers).sum(1) == 0).any()
    for get_map in (True, False):
        kw = dict(mc_samples=7, vans=VANS, get_map=get_map, lag=lag, alphabet_name=alphabet_name, no_ends=no_ends, seed=9)
        want = get_var_probs.get_bear_probs_seqs(None, queries, 0, counter=host, **kw)
        got = get_var_probs.get_bear_probs_seqs(None, queries, 0, counter=dev, **kw)
        assert got.shape == want.shape == ((len(queries), 3) if get_map else (len(queries), 3, 7))
        index, lp_abs = _table_of(kmers, host, None, None, alphabet_name, get_map, 7, 9)
        for i, s in enumerate(strings):
            n, mass = _mass([s], lag, index, lp_abs, alphabet_name)
            err = np.abs(got[i] - want[i]).reshape(mass.shape)
            assert np.all(err <= (n + 2) * U * mass), (s, n)
            assert n > 0 or not got[i].any()
        assert np.abs(want).max() > 1
    kw = dict(vans=VANS, get_marg=True, lag=lag, alphabet_name=alphabet_name, no_ends=no_ends)
    marg = get_var_probs.get_bear_probs_seqs(None, queries, 0, counter=dev, **kw)
    assert np.array_equal(marg, get_var_probs.get_bear_probs_seqs(None, queries, 0, counter=host, **kw)) and marg.shape == (len(queries), 3)


# ------------------------------------------------------------------------------------------- 7. a trained folder
def _prot_table_600(tmp_path, lag, seed):
    """600 protein k-mers, most contexts of PROT_WT among them, in a text file the protein dataloader reads."""
    rng = np.random.default_rng(seed)
    p = "[" * lag + PROT_WT + "]"
    keep = [k for k in sorted({p[j:j + lag] for j in range(len(p) - lag)}) if rng.random() < 0.8]
    while len(set(keep)) < 600:
        keep.append("".join(rng.choice(np.array(list(PROT)), lag)))
    kmers = sorted(set(keep))
    counts = np.where(rng.random((2, 600, 21)) < 0.3, rng.poisson(rng.uniform(0.5, 30, (2, 600, 1)), (2, 600, 21)), 0).astype(np.uint32)
    write_prot_tsv(tmp_path / "protk4.tsv", kmers, counts)
    return {k: counts[0, i].astype(np.float64) for i, k in enumerate(kmers)}


def test_trained_folder_scores_on_the_device(tmp_path):
    from bear_amd.models import train_bear_net
    lag = 4
    (tmp_path / "in").mkdir()
    table = _prot_table_600(tmp_path / "in", lag, seed=3)
    config = configparser.ConfigParser()
    config.read(os.path.join(ROOT, "bear_amd", "models", "config_files", "bear_test.cfg"))
    out = tmp_path / "out"
    config["general"]["out_folder"] = str(out) + "*"
    config["data"].update({"files_path": str(tmp_path / "in"), "start_token": "protk", "alphabet": "prot", "num_ds": "2",
                           "reference_column": "1"})
    config["hyperp"]["lag"] = str(lag)
    config["train"].update({"batch_size": "150", "epochs": "2", "train_ar": "False"})
    config["model"]["ar_func_name"] = "linear"
    exit_code, _, _ = train_bear_net.main(config)
    assert exit_code == 1
    _, alphabet, h, ar_func, data = get_var_probs.load_bear(str(out))
    assert alphabet == "prot" and data.num_rows == 600

    def host(kmers):
        kmers = np.asarray(kmers)
        return np.array([table.get(str(k), np.zeros(21)) for k in kmers.reshape(-1)]).reshape(kmers.shape + (21,))
    dev = get_var_probs.DeviceCounter.from_dataset(data, 0)
    assert np.array_equal(dev(sorted(table)[:50] + ["WWWW"]), host(sorted(table)[:50] + ["WWWW"]))
    kmers = get_var_probs._get_all_kmers_vars([get_var_probs.parse_var(v) for v in PROT_VARS], "[" * lag + PROT_WT + "]", lag)
    for get_map, shape in ((True, (len(PROT_VARS), 5)), (False, (len(PROT_VARS), 4, 5))):
        kw = dict(mc_samples=5, vans=VANS, get_map=get_map, seed=2)
        want = get_var_probs.get_bear_probs(str(out), PROT_WT, PROT_VARS, 0, counter=host, **kw)
        got = get_var_probs.get_bear_probs(str(out), PROT_WT, PROT_VARS, 0, counter=dev, **kw)
        assert got.shape == want.shape == shape
        lp = get_var_probs.get_pdf(kmers, host(kmers)[:, None, :], np.array([h]), ar_func, 5, VANS, 0, "prot", get_map, output="numpy",
                                   seed=2, row_base=0)
        _check_vars(got, want, PROT_WT, PROT_VARS, lag, {k: i for i, k in enumerate(kmers)}, np.abs(lp), "prot")
        assert np.abs(want).max() > 0.1


# ------------------------------------------------------------------------------------------- 8. refusals
def test_a_character_outside_the_alphabet_is_refused_before_any_launch(monkeypatch):
    dev = get_var_probs.DeviceCounter.from_sequences(DNA_SEQS, 3, alphabet_name="dna")

    def no_launch(*args):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(kernels, "_launch", no_launch)
    kw = dict(vans=VANS, lag=3, alphabet_name="dna", counter=dev, seed=1)
    with pytest.raises(ValueError, match="'N'"):
        get_var_probs.get_bear_probs(None, DNA_WT, ["A0N"], 0, **kw)
    with pytest.raises(ValueError, match="'N'"):
        get_var_probs.get_bear_probs(None, "ACNTTGCAAGTC", ["T3A"], 0, **kw)
    with pytest.raises(ValueError, match="'x'"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGT", "ACxGT"], 0, **kw)
    with pytest.raises(ValueError, match=r"'\]'"):
        get_var_probs.get_bear_probs_seqs(None, ["AC]GT"], 0, **kw)
    with pytest.raises(ValueError, match="lag"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, **dict(kw, lag=4))


# ------------------------------------------------------------------------------------------- 9. the deterministic library
_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from bear_amd import _lib, get_var_probs
import test_score_gpu as t
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
lag, wt, vars_, seqs, reverse = t.VAR_CASES["prot"]
dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=reverse, alphabet_name="prot")
np.save(sys.argv[2], t._var_call("prot", dev, False))
"""


def test_deterministic_library_returns_the_same_bytes(tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    lag, wt, vars_, seqs, reverse = VAR_CASES["prot"]
    dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=reverse, alphabet_name="prot")
    here = _var_call("prot", dev, False)
    script = tmp_path / "det_score.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npy")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    there = np.load(tmp_path / "det.npy")
    assert there.shape == here.shape and there.tobytes() == here.tobytes()
