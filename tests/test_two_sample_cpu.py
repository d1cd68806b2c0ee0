"""CPU tests of the two-sample and goodness-of-fit Bayes factors (kernels_twosample.h, bear_two_sample_f64, bear_amd.hypothesis): the
entry in the header and both libraries, its refusals before any device call, the Python refusals, the tests' own oracle, and the
statistical case the GPU tests run on the device, verified here with the SciPy twin of the oracle."""
import ctypes
import inspect

import numpy as np
import pytest

import two_sample_util as tu
from util import abi_header, stream_entries

ENTRY = "bear_two_sample_f64"


def test_entry_declared_and_bound_in_both_libraries():
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    assert version == 12 == _lib.ABI_VERSION
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    want = [vp, vp, vp, vp, u64, i, vp, i, vp, i, vp, vp, vp, vp]
    assert sigs[ENTRY] == (i, want)                                   # the tests' reader
    assert ENTRY in _lib.SYMBOLS and _lib._SIGNATURES[ENTRY] == (i, want)      # the binding's
    header = " ".join(open(_lib.HEADER_PATH).read().split())
    assert ("int bear_two_sample_f64(bear_ws *ws, const uint32_t *a, const uint32_t *b, const double *prior, uint64_t n_rows, int width, "
            "const double *h, int n_h, const double *van, int n_van, void *stream, double *out, double *out_ar, double *row_terms);") in header
    assert "#define BEAR_TWO_SAMPLE_MAX_MODELS %d" % kernels.TWO_SAMPLE_MAX_MODELS in header and kernels.TWO_SAMPLE_MAX_MODELS == 16
    assert ENTRY not in stream_entries()                              # the stream is not the last parameter (include/bear_hip.h says why)
    fn = getattr(_lib.lib(), ENTRY)
    assert fn.restype is i and list(fn.argtypes) == want
    det = ctypes.CDLL(_lib.LIB_PATH.replace("libbear_hip.so", "libbear_hip_det.so"))
    assert hasattr(det, ENTRY)
    assert list(inspect.signature(kernels.two_sample).parameters) == ["a", "b", "prior", "h", "vans", "want_ar", "want_rows", "ws"]


def _call(ws=0x100, a=0x1000, b=0x2000, prior=None, n_rows=4, width=5, h=(), van=(1.0,), n_h=None, n_van=None, out=0x4000, out_ar=None,
          row_terms=None):
    """The entry with host vectors h / van and the given (fake) addresses, which are never followed: every case returns first."""
    from bear_amd import _lib
    h, van = np.asarray(h, dtype=np.float64), np.asarray(van, dtype=np.float64)
    return _lib.lib().bear_two_sample_f64(ws, a, b, prior, n_rows, width, h.ctypes.data if h.size else None, h.size if n_h is None else n_h,
                                          van.ctypes.data if van.size else None, van.size if n_van is None else n_van, None, out, out_ar,
                                          row_terms)


def test_arguments_are_checked_before_any_device_call():
    from bear_amd import kernels
    for width in (0, 4, 6, 20, 22):
        assert _call(width=width) == -1
    assert _call(h=(1.0,)) == -1 and _call(out_ar=0x5000) == -1       # BEAR models, the AR likelihood: no prior rows
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(van=(1.0, bad)) == -1
        assert _call(h=(bad, 1.0), prior=0x3000) == -1
    assert _call(van=()) == -1 and _call(n_h=-1) == -1 and _call(n_van=-1) == -1
    assert _call(van=np.ones(kernels.TWO_SAMPLE_MAX_MODELS + 1)) == -1
    assert _call(h=np.ones(kernels.TWO_SAMPLE_MAX_MODELS), van=(1.0,), prior=0x3000) == -1
    assert _call(n_h=1) == -1 and _call(van=(), n_van=1) == -1        # a count without its values
    for name in ("ws", "a", "b", "out"):
        assert _call(**{name: None}) == -1, name
    for name, address in (("a", 0x1004), ("b", 0x2008), ("prior", 0x3004), ("out", 0x4004), ("out_ar", 0x5004), ("row_terms", 0x6004)):
        assert _call(**dict(dict(prior=0x3000), **{name: address})) == -1, name


def _no_device(monkeypatch):
    import torch
    from bear_amd import _lib, kernels

    def no_device(*args, **kwargs):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(kernels, "_stream", no_device)
    monkeypatch.setattr(kernels, "default_workspace", no_device)
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)


def test_python_refusals_need_no_device(monkeypatch):
    from bear_amd import dataloader, hypothesis
    _no_device(monkeypatch)
    kmers = np.frombuffer(b"ACGTAACGTC", dtype=np.uint8).reshape(2, 5)
    counts = np.ones((3, 2, 5), dtype=np.uint32)
    data = dataloader.CountDataset(kmers, counts, "dna", 2)

    def uniform(codes):
        raise AssertionError("the AR function was called")
    with pytest.raises(ValueError, match="sharded"):
        hypothesis.two_sample(dataloader.CountDataset(kmers[:1], counts[:, :1], "dna", 2, shard=(0, 2), total_rows=2), 0, 1, vans=[1.0])
    with pytest.raises(ValueError, match="sharded"):
        hypothesis.two_sample(data.deal_by_kmer(0, 2), 0, 1, vans=[1.0])
    with pytest.raises(ValueError, match="col_a and col_b"):
        hypothesis.two_sample(data, 1, 1, vans=[1.0])
    with pytest.raises(ValueError, match="no model"):
        hypothesis.two_sample(data, 0, 1)
    with pytest.raises(ValueError, match="no model"):
        hypothesis.two_sample_from_sequences(["ACGT"], ["ACGA"], [1])
    for kw in (dict(vans=[1.0, 0.0]), dict(vans=[-1.0]), dict(vans=[float("nan")]), dict(ar_func=uniform, h=0.0), dict(ar_func=uniform, h=[1.0, -2.0])):
        with pytest.raises(ValueError, match="> 0"):
            hypothesis.two_sample(data, 0, 1, **kw)
        with pytest.raises(ValueError, match="> 0"):
            hypothesis.two_sample_from_sequences(["ACGT"], ["ACGA"], [1], **kw)
    with pytest.raises(ValueError, match="come together"):
        hypothesis.two_sample(data, 0, 1, ar_func=uniform)
    with pytest.raises(ValueError, match="come together"):
        hypothesis.two_sample(data, 0, 1, h=1.0, vans=[1.0])
    with pytest.raises(ValueError, match="not both"):
        hypothesis.two_sample(data, 0, 1, bear_path="somewhere", ar_func=uniform, h=1.0)
    with pytest.raises(ValueError, match="at most"):
        hypothesis.two_sample(data, 0, 1, vans=np.ones(17))
    r = hypothesis.TwoSampleResult(["bear(h=1)", "van(1)"], 1, np.arange(8.0).reshape(2, 4), np.array([10.0, 20.0]), None)
    assert r.log_bf.tolist() == [3.0, 7.0] and r.log_marg.shape == (2, 3) and r.gof_log_bf().tolist() == [[-10.0, -19.0]]
    assert hypothesis.TwoSampleResult(["van(1)"], 0, np.zeros((1, 4)), None, None).gof_log_bf().shape == (0, 2)


# ------------------------------------------------------------------------------------------- the oracle
@pytest.fixture(scope="module")
def oracle5():
    a, b, prior = tu.base_rows(5)
    return a, b, prior, tu.oracle_rows(a, b, prior, tu.HS, tu.VANS)


def test_oracle_sanity(oracle5):
    a, b, prior, rows = oracle5
    val, mass = tu.as_float(rows[0]), tu.as_float(rows[1])
    na, nb = a.astype(np.uint64).sum(1), b.astype(np.uint64).sum(1)
    assert ((na > 0) & (nb > 0)).sum() > 20 and (na == 0).sum() >= 2 and (nb == 0).sum() >= 3 and ((na == 0) & (nb == 0)).any()
    assert (a.astype(np.uint64) + b > 2 ** 32).any() and (na + nb > 2 ** 34).any()
    one_side = (na == 0) | (nb == 0)
    assert all(v == 0 for v in rows[0][one_side][:, :, 3].reshape(-1))            # B_k = 0 exactly (at 50 digits) when a column is empty
    only_a = nb == 0
    assert all(x == y for x, y in zip(rows[0][only_a][:, :, 2].reshape(-1), rows[0][only_a][:, :, 0].reshape(-1)))   # M_ab = M_a
    assert np.abs(val[~one_side][:, :, 3]).min() > 0
    zb = np.zeros_like(b)
    empty = tu.oracle_sums(tu.oracle_rows(a, zb, prior, tu.HS, tu.VANS))
    assert not empty[0][:, 3].any() and not empty[0][:, 1].any() and np.array_equal(empty[0][:, 2], empty[0][:, 0]) and not empty[2][1]
    out, out_mass, ar, ar_mass = tu.oracle_sums(rows)
    sp_out, sp_ar = tu.scipy_sums(a, b, prior, tu.HS, tu.VANS)
    assert np.all(np.abs(out - sp_out) <= 1e-9 * out_mass) and np.all(np.abs(ar - sp_ar) <= 1e-9 * ar_mass)
    assert np.all(out_mass >= np.abs(out)) and np.abs(out).min() > 1.0
    # a table made of base rows sums to the multiplicities times the rows
    idx = tu.table_index(len(a), 300, seed=3)
    assert idx[0] == 0 and sorted(set(idx.tolist())) == list(range(len(a)))
    big = tu.oracle_sums(rows, idx)
    sp_big, _ = tu.scipy_sums(a[idx], b[idx], prior[idx], tu.HS, tu.VANS)
    assert np.all(np.abs(big[0] - sp_big) <= 1e-9 * big[1])


# ------------------------------------------------------------------------------------------- the statistical case
def _uniform_models(W):
    return np.array([0.05, 5.0]), np.array([1.0]), lambda n: np.full((n, W), 1.0 / W)


@pytest.mark.parametrize("alphabet", ["dna", "prot"])
def test_statistical_case_signs(alphabet):
    """Two chains with Dirichlet(0.7) rows; 100 sequences of 120 letters from the first (seeds 10 and 11) and from the second (seed
    12); van = 1 and uniform AR rows with h = 0.05 and 5: two samples of one source give a negative log Bayes factor under every
    model and lag, samples of the two sources a positive one.  'dna': chains of order 2, lags 1, 3, 5.  'prot', the 20-letter
    analogue: chains of order 1 and lags 1, 2, 3 -- 12 000 letters resolve 20 rows of 20 letters (600 transitions a row), not the
    400 rows of an order-2 chain, whose lag-1 view averages over the first letter and is nearly the same for both chains; and at
    lag 5 nearly every protein context is seen in one sample only (a term of exactly zero), too few are left to carry a sign."""
    W = len(tu.LETTERS[alphabet]) + 1
    order, lags = tu.STAT_CASE[alphabet]
    P1, P2 = tu.chain(1, alphabet, order), tu.chain(2, alphabet, order)
    s10, s11, s12 = (tu.sample_seqs(P, s, alphabet, order=order) for P, s in ((P1, 10), (P1, 11), (P2, 12)))
    hs, vans, rows = _uniform_models(W)
    for lag in lags:
        for other, sign in ((s11, -1), (s12, +1)):
            a, b = tu.count_host(s10, other, lag, alphabet)
            out, ar = tu.scipy_sums(a, b, rows(len(a)), hs, vans)
            print(f"{alphabet} lag {lag} {'same' if sign < 0 else 'different'} source: log BF {out[:, 3]}")
            assert np.all(np.sign(out[:, 3]) == sign), (alphabet, lag, sign, out[:, 3])
            assert a.sum() == b.sum() == 100 * 121 and np.all(np.isfinite(ar))
