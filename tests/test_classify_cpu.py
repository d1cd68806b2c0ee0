"""CPU tests of the group classifier (kernels_groups.h, bear_score_groups_f64, bear_amd.classify): the entry in the header, the
binding and both libraries, its refusals before any device call, the refusals of the Python layers without a device, and the
oracle of tests/classify_util.py against itself."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import classify_util as cu
from util import abi_header

ENTRY = "bear_score_groups_f64"
STREAM_ARG = 15


def test_entry_declared_with_the_stream_in_position_15_and_exported_by_both_libraries():
    from bear_amd import _lib, kernels
    _, sigs = abi_header()
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    want = [vp, vp, u64, vp, u64, i, vp, i, vp, u64, vp, vp, i, vp, i, vp, vp, vp]
    assert ENTRY in _lib.SYMBOLS and sigs[ENTRY] == (i, want) and _lib._SIGNATURES[ENTRY] == (i, want)
    header = open(_lib.HEADER_PATH).read()
    decl = re.search(r"^int %s\(([^)]*)\);" % ENTRY, header, flags=re.M | re.S)
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert len(params) == 18 and params[STREAM_ARG] == "void *stream" and params[-2:] == ["double *scores", "uint8_t *short_of"]
    assert params[7] == "int n_groups" and params[10] == "const int32_t *own"
    assert "#define BEAR_GROUPS_MAX %d" % kernels.GROUPS_MAX in header and kernels.GROUPS_MAX == 256
    fn = getattr(_lib.lib(), ENTRY)
    assert fn.restype is i and list(fn.argtypes) == want
    det = ctypes.CDLL(_lib.LIB_PATH.replace("libbear_hip.so", "libbear_hip_det.so"))
    assert hasattr(det, ENTRY)
    assert list(inspect.signature(kernels.score_groups).parameters) == ["rows", "letters", "seg", "train", "prior", "h", "vans", "own"]


def _call(width=5, prior=None, K=10, G=3, h=(), van=(0.1, 1.0), n_seg=0, n_h=None, n_van=None, rows=None, letters=None, n_t=0, seg=None,
          train=None, own=None, scores=None, short_of=None):
    """The entry with host vectors h / van and the given (fake) device addresses: every case here returns before a device call."""
    from bear_amd import _lib
    h, van = np.asarray(h, dtype=np.float64), np.asarray(van, dtype=np.float64)
    return _lib.lib().bear_score_groups_f64(rows, letters, n_t, seg, n_seg, width, train, G, prior, K, own,
                                            h.ctypes.data if h.size else None, h.size if n_h is None else n_h,
                                            van.ctypes.data if van.size else None, van.size if n_van is None else n_van, None, scores, short_of)


def test_arguments_are_checked_before_any_device_call():
    from bear_amd import kernels
    assert _call() == 0                                               # n_seg == 0: nothing to launch
    assert _call(width=21, h=(0.05, 3.0), prior=0x1000, G=kernels.GROUPS_MAX) == 0
    for G in (0, -1, kernels.GROUPS_MAX + 1):
        assert _call(G=G) == -1
    # everything bear_score_marg_f64 refuses (tests/test_marg_cpu.py)
    for width in (0, 4, 6, 20, 22):
        assert _call(width=width) == -1
    assert _call(h=(1.0,), prior=None) == -1
    for bad in (0.0, -1.0, float("nan")):
        assert _call(van=(1.0, bad)) == -1
        assert _call(h=(bad, 1.0), prior=0x1000) == -1
    assert _call(van=()) == -1
    assert _call(van=np.ones(kernels.MARG_MAX_MODELS)) == 0 and _call(van=np.ones(kernels.MARG_MAX_MODELS + 1)) == -1
    assert _call(n_h=-1) == -1 and _call(n_van=-1) == -1
    assert _call(K=2 ** 32 - 1) == -1 and _call(K=2 ** 32 - 2) == 0
    assert _call(own=0x6002) == -1 and _call(own=0x6004) == 0        # a misaligned own, with or without segments
    ok = dict(n_seg=1, n_t=4, rows=0x1000, letters=0x1001, seg=0x2000, train=0x3000, own=0x6000, scores=0x4000, short_of=0x5001)
    for name in ("rows", "letters", "seg", "train", "scores", "short_of"):
        assert _call(**dict(ok, **{name: None})) == -1, name
    for name, address in (("rows", 0x1002), ("seg", 0x2004), ("train", 0x3002), ("scores", 0x4004), ("own", 0x6002)):
        assert _call(**dict(ok, **{name: address})) == -1, name
    assert _call(**dict(ok, h=(1.0,), prior=0x5004)) == -1


def _hollow_counter(G=3, reverse=False, alphabet="dna", lag=2):
    """A GroupCounter that holds no table: every refusal below comes before it is looked at."""
    import torch
    from bear_amd import classify
    counter = object.__new__(classify.GroupCounter)
    counter.counts = torch.zeros((0, G, 5 if alphabet == "dna" else 21), dtype=torch.int32)
    counter.lag, counter.alphabet_name, counter.reverse = lag, alphabet, reverse
    return counter


def test_python_refusals_need_no_device(monkeypatch):
    import torch
    from bear_amd import classify, dataloader, get_var_probs, kernels, _lib

    def no_device(*args, **kwargs):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(kernels, "_launch", no_device)
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(get_var_probs, "_device", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    assert list(inspect.signature(classify.classify).parameters) == ["counter", "seqs", "vans", "bear_path", "ar_func", "h", "log_prior",
                                                                     "own_group", "no_ends"]
    assert all(p.kind is p.KEYWORD_ONLY for p in list(inspect.signature(classify.classify).parameters.values())[2:])
    counter = _hollow_counter()

    def uniform(codes):
        raise AssertionError("the AR function was called")
    # the refusals of hypothesis._check_model
    for kw in (dict(), dict(ar_func=uniform), dict(h=1.0), dict(bear_path="somewhere", ar_func=uniform, h=1.0), dict(vans=[1.0, 0.0]),
               dict(vans=[float("inf")]), dict(ar_func=uniform, h=[1.0, -2.0]), dict(vans=np.ones(17))):
        with pytest.raises(ValueError):
            classify.classify(counter, ["ACGT"], **kw)
    with pytest.raises(ValueError, match="GroupCounter"):
        classify.classify(object.__new__(get_var_probs.DeviceCounter), ["ACGT"], vans=[1.0])
    for bad in (np.zeros(2), np.zeros((3, 1)), [0.0, float("nan"), 0.0], [0.0, float("inf"), 0.0]):
        with pytest.raises(ValueError, match="log_prior"):
            classify.classify(counter, ["ACGT"], vans=[1.0], log_prior=bad)
    for bad in ([0], [0, 1, 2], [0.0, 1.0], [0, 3], [-2, 0]):
        with pytest.raises(ValueError, match="own_group"):
            classify.classify(counter, ["ACGT", "AC"], vans=[1.0], own_group=bad)
    with pytest.raises(ValueError, match="reverse=True"):
        classify.classify(_hollow_counter(reverse=True), ["ACGT", "AC"], vans=[1.0], own_group=[0, -1])
    # the tables GroupCounter refuses
    kmers = np.frombuffer(b"ACCAGT", dtype=np.uint8).reshape(3, 2)
    counts = np.ones((2, 3, 5), dtype=np.uint32)
    data = dataloader.CountDataset(kmers, counts, "dna", 2)
    with pytest.raises(ValueError, match="sharded"):
        classify.GroupCounter.from_dataset(dataloader.CountDataset(kmers[:1], counts[:, :1], "dna", 2, shard=(0, 2), total_rows=3))
    with pytest.raises(ValueError, match="sharded"):
        classify.GroupCounter.from_dataset(data.deal_by_kmer(0, 2))
    for cols in ([], [2], [0, -1]):
        with pytest.raises(ValueError, match="cols"):
            classify.GroupCounter.from_dataset(data, cols=cols)
    with pytest.raises(ValueError, match="CountDataset"):
        classify.GroupCounter.from_dataset(counts)
    with pytest.raises(ValueError, match="reverse"):
        classify.GroupCounter.from_sequences([["MKT"], ["MKV"]], 2, alphabet_name="prot", reverse=True)
    with pytest.raises(ValueError, match="one per group"):
        classify.GroupCounter.from_sequences(["ACGT", "ACGA"], 2)
    with pytest.raises(ValueError, match="one per group"):
        classify.GroupCounter.from_sequences([], 2)
    # kernels.score_groups: what is checked before the first launch
    cpu = torch.zeros((4, 3, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="train"):
        kernels.score_groups(None, None, None, cpu, None, None, [1.0])
    with pytest.raises(ValueError, match="train"):
        kernels.score_groups(None, None, None, torch.zeros((4, 5), dtype=torch.int32), None, None, [1.0])


def test_pieces_are_whole_sequences_within_the_budget():
    from bear_amd import classify
    assert classify._pieces([], 8, 100) == []
    assert classify._pieces([5, 5, 5, 5, 5], 8, 80) == [(0, 2), (2, 4), (4, 5)]
    assert classify._pieces([5, 50, 5], 8, 80) == [(0, 1), (1, 2), (2, 3)]           # a sequence beyond the budget goes alone
    assert classify._pieces([3, 3, 3], 8, 10 ** 9) == [(0, 3)]


# ------------------------------------------------------------------------------------------- the oracle against itself
@pytest.mark.parametrize("alphabet", ["dna", "prot"])
def test_oracle_leave_one_out_is_the_plain_formula_on_the_table_less_the_sequence(alphabet):
    import two_sample_util as tu
    lag, W = 2, len(tu.LETTERS[alphabet]) + 1
    groups = [tu.sample_seqs(tu.chain(7 + g, alphabet, 1), 70 + g, alphabet, n_seqs=4, length=30, order=1) for g in range(3)]
    table = cu.count_host(groups, lag, alphabet)
    rng = np.random.default_rng(5)
    prior = {k: rng.dirichlet(np.full(W, 0.5)) + 1e-7 for k in table}
    strings = ["[" * lag + s + "]" for seqs in groups for s in seqs]
    own = np.repeat([0, 1, 2], 4)
    loo, mass = cu.oracle(cu.string_entries(strings, lag, alphabet, table, 3, prior.get), cu.HS, cu.VANS, W, 3, own)
    plain, _ = cu.oracle(cu.string_entries(strings, lag, alphabet, table, 3, prior.get), cu.HS, cu.VANS, W, 3)
    assert np.isfinite(loo).all() and np.abs(loo).min() > 1
    for i, s in enumerate(strings):
        less = {k: v.copy() for k, v in table.items()}
        for p in range(lag, len(s)):
            less[s[p - lag:p]][own[i], (tu.LETTERS[alphabet] + "]").index(s[p])] -= 1
        want, _ = cu.oracle(cu.string_entries([s], lag, alphabet, less, 3, prior.get), cu.HS, cu.VANS, W, 3)
        assert np.array_equal(loo[i], want[0])                          # the same 50-digit sums, rounded once
        others = np.arange(3) != own[i]
        assert np.array_equal(loo[i, others], plain[i, others]) and np.all(loo[i, own[i]] != plain[i, own[i]])
    # a sequence that its claimed group does not hold: NaN there, and only there
    lost, _ = cu.oracle(cu.string_entries(strings[:1], lag, alphabet, table, 3, prior.get), cu.HS, cu.VANS, W, 3, [1])
    assert np.isnan(lost[0, 1]).all() and np.array_equal(lost[0, [0, 2]], plain[0, [0, 2]])


def test_oracle_posterior():
    rng = np.random.default_rng(1)
    one = cu.log_post(rng.normal(-50, 10, (4, 1, 3)))
    assert one.shape == (4, 1, 3) and not one.any()                      # G = 1: log_post == 0
    marg = rng.normal(-50, 3, (5, 3, 2))
    post = cu.log_post(marg)
    assert np.allclose(np.exp(post).sum(1), 1.0, rtol=0, atol=1e-15)
    shifted = cu.log_post(marg, np.log([0.2, 0.3, 0.5]))
    want = marg + np.log([0.2, 0.3, 0.5])[None, :, None]
    assert np.allclose(shifted - shifted[:, :1], want - want[:, :1], rtol=0, atol=1e-12)
    assert np.allclose(cu.log_post(marg, [3.0, 3.0, 3.0]), post, rtol=0, atol=1e-13)      # a common shift cancels


def test_statistical_case_is_decided_by_the_oracle_alone():
    """The seeds of classify_util.STAT_SEEDS were chosen here, with the oracle alone: no held-out sequence within 1e-6 of a tie and
    an accuracy of at least 0.9 (dna lag 1: 0.995; dna lag 2, prot lag 1 and 2: 1.0)."""
    for alphabet in ("dna", "prot"):
        for lag in cu.STAT_LAGS:
            _, margin, accuracy = cu.stat_oracle(alphabet, lag)
            assert (margin > 1e-6).all() and accuracy >= 0.9, (alphabet, lag, accuracy)
