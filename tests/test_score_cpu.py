"""CPU tests of scoring on the device (get_var_probs.DeviceCounter, kernels_score.h): the rank table that makes look-up keys sort
as Python sorts k-mer strings, the class and its constructors, and the three entries in the header and the binding."""
import ctypes
import inspect

import numpy as np
import pytest

from util import abi_header

ENTRIES = ("bear_score_transitions_u64", "bear_kmer_find_u64", "bear_score_sum_f64")


def _pack(kmer, alphabet_name, rank):
    """The key of a k-mer, restated: the ranks of its characters, first letter most significant, SCORE_BITS[W] bits each."""
    from bear_amd import core, kernels
    letters = [str(c) for c in core.alphabets_en[alphabet_name][:-1]]
    W = len(letters) + 1
    code = {ch: c for c, ch in enumerate(letters)}
    code["["] = W                                                     # the start symbol's code; W - 1 is the stop
    key = 0
    for ch in kmer:
        key = (key << kernels.SCORE_BITS[W]) | int(rank[code[ch]])
    return key


@pytest.mark.parametrize("alphabet_name,lags", [("dna", (1, 5, 21)), ("rna", (1, 8, 21)), ("prot", (1, 4, 12))])
def test_rank_packed_keys_sort_as_the_strings(alphabet_name, lags):
    from bear_amd import core, kernels
    rank = kernels.score_ranks(alphabet_name)
    letters = [str(c) for c in core.alphabets_en[alphabet_name][:-1]]
    W = len(letters) + 1
    assert rank.dtype == np.uint8 and rank.shape == (W + 1,) and rank[W - 1] == 0xFF          # the stop is no letter of a context
    chars = sorted(letters + ["["])
    assert [int(rank[c]) for c in range(W - 1)] == [chars.index(ch) for ch in letters] and int(rank[W]) == chars.index("[")
    assert max(int(r) for r in rank if r != 0xFF) < 1 << kernels.SCORE_BITS[W]
    rng = np.random.default_rng(len(alphabet_name))
    for lag in lags:
        assert lag <= kernels.SCORE_MAX_LAG[W] and kernels.SCORE_BITS[W] * lag < 64
        kmers = {"".join(rng.choice(letters + ["["], lag)) for _ in range(400)} | {"[" * lag, letters[0] * lag, letters[-1] * lag}
        # padded contexts as they occur: '[' only in front
        kmers |= {"[" * j + "".join(rng.choice(letters, lag - j)) for j in range(lag + 1) for _ in range(5)}
        kmers = list(kmers)
        keys = [_pack(k, alphabet_name, rank) for k in kmers]
        assert len(set(keys)) == len(kmers) and max(keys) < 1 << 63
        assert [k for _, k in sorted(zip(keys, kmers))] == sorted(kmers)
        assert np.array_equal(np.array(sorted(set(kmers))), np.array(kmers)[np.argsort(np.array(keys, dtype=np.uint64))])


def test_device_counter_has_both_constructors():
    from bear_amd import get_var_probs
    cls = get_var_probs.DeviceCounter
    assert callable(cls.from_sequences) and callable(cls.from_dataset) and callable(cls.__call__)
    seq_args = list(inspect.signature(cls.from_sequences).parameters)
    assert seq_args == list(inspect.signature(get_var_probs.make_sequence_counter).parameters)
    assert list(inspect.signature(cls.from_dataset).parameters)[:2] == ["data", "train_col"]
    with pytest.raises(ValueError):
        cls.from_sequences(["ACDE"], 2, reverse=True, alphabet_name="prot")        # no reverse complement, as make_sequence_counter


def test_text_refusals_need_no_device():
    """What the kernels would make no key of is a ValueError that names the character, raised before anything is launched."""
    from bear_amd import get_var_probs
    codes, seg, none = get_var_probs._segment_text(["[[AC]", "[[]", "[", ""], 2, "dna")
    assert codes.tolist() == [5, 5, 0, 1, 4, 5, 5, 4, 5] and seg.tolist() == [0, 5, 8, 9, 9] and none == 2 + 2 + 1 + 0
    for bad, ch in ((["[[ANT]"], "'N'"), (["[[AC]", "[[a]"], "'a'"), (["[[A]C]"], "']'"), (["[[A[C]"], "'['"), (["[[Aé]"], "'é'")):
        with pytest.raises(ValueError, match=".*" + ch.replace("[", r"\[").replace("]", r"\]")):
            get_var_probs._segment_text(bad, 2, "dna")
    get_var_probs._segment_text(["AC]"], 3, "dna")              # no transition: the stop is in no context
    with pytest.raises(ValueError):
        get_var_probs._segment_text(["[[[MKB]"], 3, "prot")


def test_entries_declared_and_bound():
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    assert version == 12 == _lib.ABI_VERSION
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    want = {"bear_score_transitions_u64": [vp, vp, u64, u64, i, i, vp, vp, vp, vp],
            "bear_kmer_find_u64": [vp, u64, vp, u64, vp, vp],
            "bear_score_sum_f64": [vp, u64, i, u64, vp, vp, u64, vp, u64, vp, vp]}
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and sigs[name] == (i, want[name])
        fn = getattr(L, name)
        assert fn.restype is i and list(fn.argtypes) == want[name]
    for name in ("score_transitions", "kmer_find", "score_sum", "score_ranks"):
        assert callable(getattr(kernels, name))
    header = open(_lib.HEADER_PATH).read()
    assert "#define BEAR_SCORE_CHUNK %d" % kernels.SCORE_CHUNK in header
    # arguments are checked before any device call
    assert L.bear_kmer_find_u64(None, 2 ** 32 - 1, None, 0, None, None) == -1
    assert L.bear_kmer_find_u64(None, 0, None, 0, None, None) == 0
    assert L.bear_score_sum_f64(None, 0, 7, 1, None, None, 0, None, 0, None, None) == -1
    rank = kernels.score_ranks("dna")
    assert L.bear_score_transitions_u64(None, None, 0, 0, 22, 5, rank.ctypes.data, None, None, None) == -1
    assert L.bear_score_transitions_u64(None, None, 0, 0, 21, 5, rank.ctypes.data, None, None, None) == 0
    assert L.bear_score_transitions_u64(None, None, 0, 0, 13, 21, kernels.score_ranks("prot").ctypes.data, None, None, None) == -1
