"""CPU tests of the exact posterior mean and variance of scores (kernels_moments.h, bear_score_moments_f64, ``moments=True`` of
get_bear_probs / get_bear_probs_seqs): the entry and the probe operations in the header and the binding, the entry's refusals before
any device call, the keyword's refusals, the signed segments a variant becomes, and the two formulas against a Dirichlet sample."""
import ctypes
import inspect

import numpy as np
import pytest
from scipy import special

from util import abi_header

ENTRY = "bear_score_moments_f64"


def test_entry_and_probe_operations_declared_and_bound():
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    assert version == 12 == _lib.ABI_VERSION
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    want = [vp, vp, vp, u64, vp, u64, i, vp, vp, u64, vp, i, vp, i, vp, vp]
    assert ENTRY in _lib.SYMBOLS and sigs[ENTRY] == (i, want)
    fn = getattr(_lib.lib(), ENTRY)
    assert fn.restype is i and list(fn.argtypes) == want
    assert callable(kernels.score_moments)
    header = open(_lib.HEADER_PATH).read()
    for line in ("#define BEAR_PROBE_PSI 18", "#define BEAR_PROBE_PSI1 19", "#define BEAR_PROBE_N_OPS 20"):
        assert line + "\n" in header
    assert kernels.PROBE_OPS["psi"] == 18 and kernels.PROBE_OPS["psi1"] == 19 and len(kernels.PROBE_OPS) == 20
    assert "psi" not in kernels.PROBE_ITEM_OPS and "psi1" not in kernels.PROBE_ITEM_OPS
    det = ctypes.CDLL(_lib.LIB_PATH.replace("libbear_hip.so", "libbear_hip_det.so"))
    assert hasattr(det, ENTRY)


def _call(width=5, prior=None, K=10, h=(), van=(0.1, 1.0), n_seg=0, n_h=None, n_van=None, rows=None, letters=None, prefix=None, n_t=0,
          seg=None, train=None, moments=None):
    """The entry with host vectors h / van and the given (fake) device addresses: every case here returns before a device call."""
    from bear_amd import _lib
    h, van = np.asarray(h, dtype=np.float64), np.asarray(van, dtype=np.float64)
    return _lib.lib().bear_score_moments_f64(rows, letters, prefix, n_t, seg, n_seg, width, train, prior, K,
                                             h.ctypes.data if h.size else None, h.size if n_h is None else n_h,
                                             van.ctypes.data if van.size else None, van.size if n_van is None else n_van, moments, None)


def test_arguments_are_checked_before_any_device_call():
    """The checks and status codes of bear_score_marg_f64 (tests/test_marg_cpu.py), and the prefix's alignment."""
    from bear_amd import kernels
    assert _call() == 0                                               # n_seg == 0: nothing to launch
    assert _call(width=21, h=(0.05, 3.0), prior=0x1000) == 0
    for width in (0, 4, 6, 20, 22):
        assert _call(width=width) == -1
    assert _call(h=(1.0,), prior=None) == -1                          # BEAR models without prior rows
    assert _call(h=(1.0,), prior=0x1000) == 0
    for bad in (0.0, -1.0, float("nan")):
        assert _call(van=(1.0, bad)) == -1
        assert _call(h=(bad, 1.0), prior=0x1000) == -1
    assert _call(van=()) == -1                                        # no model at all
    assert _call(van=np.ones(kernels.MARG_MAX_MODELS)) == 0
    assert _call(van=np.ones(kernels.MARG_MAX_MODELS + 1)) == -1      # 17 models
    assert _call(h=np.ones(kernels.MARG_MAX_MODELS), van=(1.0,), prior=0x1000) == -1
    assert _call(n_h=-1) == -1 and _call(n_van=-1) == -1
    assert _call(K=2 ** 32 - 1) == -1 and _call(K=2 ** 32 - 2) == 0
    assert _call(prefix=0x6004) == -1 and _call(prefix=0x6008) == 0
    # pointers, with a segment to score: missing, then misaligned (addresses that are never followed)
    ok = dict(n_seg=1, n_t=4, rows=0x1000, letters=0x1001, seg=0x2000, train=0x3000, moments=0x4000)
    for name in ("rows", "letters", "seg", "train", "moments"):
        assert _call(**dict(ok, **{name: None})) == -1, name
    for name, address in (("rows", 0x1002), ("seg", 0x2004), ("train", 0x3002), ("moments", 0x4004), ("prefix", 0x6004)):
        assert _call(**dict(ok, **{name: address})) == -1, name
    assert _call(**dict(ok, h=(1.0,), prior=0x5004)) == -1


def test_keyword_and_its_refusals_need_no_device(monkeypatch):
    import torch
    from bear_amd import get_var_probs, kernels
    for fn in (get_var_probs.get_bear_probs, get_var_probs.get_bear_probs_seqs):
        assert inspect.signature(fn).parameters["moments"].default is False
    assert callable(get_var_probs._moment_segments)
    assert inspect.signature(get_var_probs._moment_segments).parameters["pair"].default is False

    def no_device(*args, **kwargs):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(kernels, "_launch", no_device)
    monkeypatch.setattr(get_var_probs, "_device", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    kw = dict(vans=[0.1, 1.0], lag=3, alphabet_name="dna", moments=True)

    def plain_counter(kmers):
        return np.zeros(np.asarray(kmers).shape + (5,))
    dev = object.__new__(get_var_probs.DeviceCounter)             # a DeviceCounter that holds nothing: it must not be looked at
    for counter in (plain_counter, None):
        with pytest.raises(ValueError, match="DeviceCounter"):
            get_var_probs.get_bear_probs(None, "ACGTACGT", ["A0C"], 0, counter=counter, **kw)
        with pytest.raises(ValueError, match="DeviceCounter"):
            get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, counter=counter, **kw)
    with pytest.raises(ValueError, match="get_map"):
        get_var_probs.get_bear_probs(None, "ACGTACGT", ["A0C"], 0, counter=dev, get_map=True, **kw)
    for other in ("get_map", "get_marg", "marg_on_device"):
        with pytest.raises(ValueError, match=other):
            get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, counter=dev, **dict(kw, **{other: True}))
    with pytest.raises(ValueError, match="get_marg, marg_on_device"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, counter=dev, get_marg=True, marg_on_device=True, **kw)


def test_a_variant_is_one_signed_segment():
    """An insertion, a deletion, a substitution at position 0 and one at the last residue: the windows in pairs, the coarse offsets,
    the weights, and every transition inside one window (the first ``lag`` symbols of EVERY window hold none)."""
    from bear_amd import get_var_probs as g
    lag, wt = 3, "ACGTTGCA"
    padded = lag * "[" + wt + "]"
    variants = ["A0T", "A7G", "G2GTT", "GTT2G", "T3T"]
    vars_ = [g.parse_var(v) for v in variants]
    windows = g._variant_windows(vars_, padded, lag)
    assert windows == ["[[[TCGT", "[[[ACGT",           # substitution at position 0: the context is the padding
                       "TGCG]", "TGCA]",               # ... at the last residue: the window ends with the stop
                       "[ACGTTTTG", "[ACGTTG",         # insertion: the mutant window is longer
                       "[ACGGCA", "[ACGTTGCA",         # deletion: shorter
                       "ACGTTGC", "ACGTTGC"]           # equal to the wild type
    codes, seg, n_none = g._segment_text(windows, lag, "dna")
    assert seg.tolist() == np.r_[0, np.cumsum([len(w) for w in windows])].tolist() and n_none == lag * len(windows)
    coarse, weights = g._signed_pairs(seg)
    assert coarse.dtype == np.int64 and weights.dtype == np.int8 and weights.size == codes.size == seg[-1]
    assert coarse.tolist() == seg[0::2].tolist() and coarse[0] == 0 and coarse[-1] == codes.size and coarse.size == len(variants) + 1
    for i in range(len(variants)):
        assert (weights[seg[2 * i]:seg[2 * i + 1]] == 1).all() and (weights[seg[2 * i + 1]:seg[2 * i + 2]] == -1).all()
    # the transitions under the windows' own offsets: position p of window w holds one iff p >= lag -- what the k+1-mers of the
    # window are, none of them made of symbols of two windows; under the coarse offsets the wild type's first `lag` would hold some
    pos = np.arange(codes.size) - np.repeat(seg[:-1], np.diff(seg))
    n_trans = int((pos >= lag).sum())
    assert n_trans == sum(len(w) - lag for w in windows)
    pos_coarse = np.arange(codes.size) - np.repeat(coarse[:-1], np.diff(coarse))
    assert int((pos_coarse >= lag).sum()) == n_trans + lag * len(variants)
    # the signed multiplicities of the k+1-mers: the variant equal to the wild type cancels cell by cell, a substitution's first
    # transition has M = 0 with m = +1 and -1
    def signed(i):
        m = {}
        for w, sgn in ((windows[2 * i], 1), (windows[2 * i + 1], -1)):
            for p in range(lag, len(w)):
                m[w[p - lag:p + 1]] = m.get(w[p - lag:p + 1], 0) + sgn
        return {k: v for k, v in m.items() if v}
    assert signed(4) == {}
    assert signed(0)["[[[T"] == 1 and signed(0)["[[[A"] == -1 and sum(signed(0).values()) == 0


def _closed_form(a, m):
    """E and Var of sum_b m_b log p_b, p ~ Dirichlet(a): the two formulas, in NumPy / SciPy."""
    a, m = np.asarray(a, dtype=np.float64), np.asarray(m, dtype=np.float64)
    A, M = a.sum(), m.sum()
    mean = (m * special.digamma(a)).sum() - M * special.digamma(A)
    var = (m * m * special.polygamma(1, a)).sum() - M * M * special.polygamma(1, A)
    return mean, var


@pytest.mark.parametrize("a,m", [((0.3, 2.0, 5.5, 0.1, 7.0), (2, -1, 0, 1, 0)),
                                 ((1.5, 0.5, 4.0, 2.5, 0.75), (1, -1, 0, 2, -2)),           # M = 0
                                 (tuple(0.5 + 0.25 * np.arange(21)), tuple([3, 0, -1] * 7))])
def test_formulas_against_a_dirichlet_sample(a, m):
    n = 2_000_000
    mean, var = _closed_form(a, m)
    rng = np.random.default_rng(11)
    p = rng.dirichlet(np.asarray(a), size=n)
    assert p.min() > 0                                                    # (the smallest concentration here is 0.1: no underflow)
    s = np.log(p, out=p) @ np.asarray(m, dtype=np.float64)
    assert abs(s.mean() - mean) <= 6 * np.sqrt(var / n)
    # the sample variance against the formula's: its standard error from the sample's own fourth moment
    d2 = (s - s.mean()) ** 2
    assert abs(d2.mean() - var) <= 6 * d2.std() / np.sqrt(n)
    if sum(m) == 0:
        assert np.isclose(mean, (np.asarray(m) * special.digamma(np.asarray(a))).sum(), rtol=0, atol=1e-12)
