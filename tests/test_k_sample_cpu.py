"""CPU tests of the k-sample Bayes factors and the clustering of samples (kernels_ksample.h, bear_k_sample_f64, bear_amd.hypothesis):
the entry in the header and both libraries, its refusals before any device call, the Python refusals, the tests' own oracle against
tests/two_sample_util.py's and against its SciPy twin, and the merge loop of ``agglomerate`` driven by that twin on the six-group
statistical case the GPU tests run on the device."""
import ctypes
import inspect

import numpy as np
import pytest

import k_sample_util as ku
import two_sample_util as tu
from util import abi_header, stream_entries

ENTRY, QUERY = "bear_k_sample_f64", "bear_k_sample_scratch"


def test_entry_declared_and_bound_in_both_libraries():
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    assert version == 12 == _lib.ABI_VERSION
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    want = [vp, vp, vp, i, vp, u64, i, vp, i, vp, i, vp, vp, u64, vp, vp, vp, vp, vp]
    assert sigs[ENTRY] == (i, want) and sigs[QUERY] == (u64, [vp, u64, i, i])
    assert _lib._SIGNATURES[ENTRY] == (i, want) and _lib._SIGNATURES[QUERY] == (u64, [vp, u64, i, i])
    header = " ".join(open(_lib.HEADER_PATH).read().split())
    assert ("int bear_k_sample_f64(bear_ws *ws, const uint32_t *counts, const uint64_t *col_rows, int n_groups, const double *prior, "
            "uint64_t n_rows, int width, const double *h, int n_h, const double *van, int n_van, void *stream, double *scratch, "
            "uint64_t n_scratch, double *out_group, double *out_pair, double *out_all, double *out_ar, double *row_terms);") in header
    assert "uint64_t bear_k_sample_scratch(bear_ws *ws, uint64_t n_rows, int width, int n_groups);" in header
    assert "#define BEAR_K_SAMPLE_MAX_GROUPS %d" % kernels.K_SAMPLE_MAX_GROUPS in header and kernels.K_SAMPLE_MAX_GROUPS == 16
    assert ENTRY not in stream_entries()                              # the stream is not the last parameter (include/bear_hip.h says why)
    for path in (_lib.LIB_PATH, _lib.LIB_PATH.replace("libbear_hip.so", "libbear_hip_det.so")):
        L = ctypes.CDLL(path)
        assert hasattr(L, ENTRY) and hasattr(L, QUERY), path
    fn = getattr(_lib.lib(), ENTRY)
    assert fn.restype is i and list(fn.argtypes) == want
    assert list(inspect.signature(kernels.k_sample).parameters) == ["counts", "cols", "prior", "h", "vans", "want_ar", "want_rows", "ws"]
    assert set(kernels.K_SAMPLE_TILE) == set(kernels.WIDE_WIDTHS) and kernels.K_SAMPLE_BLOCKS_PER_CU >= 2
    for W in kernels.WIDE_WIDTHS:
        assert kernels.k_sample_tile(W, 16) == kernels.k_sample_tile(W, 9) == kernels.K_SAMPLE_TILE[W] < kernels.k_sample_tile(W, 8)


def _query(n_rows=4, width=5, n_groups=2):
    from bear_amd import _lib
    return int(_lib.lib().bear_k_sample_scratch(None, n_rows, width, n_groups))


def test_scratch_query_needs_no_device():
    from bear_amd import kernels
    assert _query(width=6) == 0 and _query(n_groups=1) == 0 and _query(n_groups=17) == 0
    for W in kernels.WIDE_WIDTHS:
        for G in (2, 3, 4, 5, 8, 9, 16):
            tile = kernels.k_sample_tile(W, G)
            one = _query(1, W, G)
            assert one > 0 and _query(0, W, G) == one == _query(tile, W, G)            # one block's sums
            assert _query(tile + 1, W, G) == 2 * one and _query(1 << 40, W, G) == _query(1 << 41, W, G)             # capped
    # at G = 16 a block leaves 4 models x (16 group sums + 2 x 120 pair sums + 2 all-groups sums) and the 16 AR sums, padded
    assert _query(1, 21, 16) >= 4 * 258 + 16


def _call(ws=0x100, counts=0x1000, cols=(0, 8), prior=None, n_rows=4, width=5, h=(), van=(1.0,), n_h=None, n_van=None, scratch=0x8000,
          n_scratch=None, out_group=0x4000, out_pair=0x5000, out_all=0x6000, out_ar=None, row_terms=None, n_groups=None, no_cols=False):
    """The entry with host vectors and the given (fake) addresses, which are never followed: every case returns first."""
    from bear_amd import _lib
    h, van, cols = np.asarray(h, dtype=np.float64), np.asarray(van, dtype=np.float64), np.asarray(cols, dtype=np.uint64)
    G = cols.size if n_groups is None else n_groups
    if n_scratch is None:
        n_scratch = _query(n_rows, width, G)
    return _lib.lib().bear_k_sample_f64(ws, counts, None if no_cols else cols.ctypes.data, G, prior, n_rows, width,
                                        h.ctypes.data if h.size else None, h.size if n_h is None else n_h,
                                        van.ctypes.data if van.size else None, van.size if n_van is None else n_van, None, scratch,
                                        n_scratch, out_group, out_pair, out_all, out_ar, row_terms)


def test_arguments_are_checked_before_any_device_call():
    from bear_amd import kernels
    # --- everything bear_two_sample_f64 refuses
    for width in (0, 4, 6, 20, 22):
        assert _call(width=width) == -1
    assert _call(h=(1.0,)) == -1 and _call(out_ar=0x7000) == -1       # BEAR models, the AR likelihood: no prior rows
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(van=(1.0, bad)) == -1
        assert _call(h=(bad, 1.0), prior=0x3000) == -1
    assert _call(van=()) == -1 and _call(n_h=-1) == -1 and _call(n_van=-1) == -1
    assert _call(van=np.ones(kernels.TWO_SAMPLE_MAX_MODELS + 1)) == -1
    assert _call(h=np.ones(kernels.TWO_SAMPLE_MAX_MODELS), van=(1.0,), prior=0x3000) == -1
    assert _call(n_h=1) == -1 and _call(van=(), n_van=1) == -1        # a count without its values
    for name in ("ws", "counts", "out_group", "out_pair", "out_all", "scratch"):
        assert _call(**{name: None}) == -1, name
    assert _call(no_cols=True) == -1
    # --- the number of groups
    for G in (-1, 0, 1, 17, 1 << 20):
        assert _call(cols=np.arange(16) * 8, n_groups=G, n_scratch=1 << 30) == -1, G
    assert _call(cols=np.arange(17) * 8, n_scratch=1 << 30) == -1
    # --- the scratch: one value short of the query, at two and at sixteen groups
    for cols in ((0, 8), np.arange(16) * 8):
        for n_rows in (0, 4, 5000):
            assert _call(cols=cols, n_rows=n_rows, n_scratch=_query(n_rows, 5, len(cols)) - 1) == -1
    assert _call(n_scratch=0) == -1
    # --- alignment: a column that starts off a 16-byte boundary (5 dwords a row: rows 4 k are on one), the outputs, the prior
    for cols in ((0, 1), (0, 6), (3, 8), (4, 8, 13)):
        assert _call(cols=cols) == -1, cols
    assert _call(counts=0x1004) == -1 and _call(counts=0x1004, cols=(4, 8)) == -1
    for name, address in (("prior", 0x3004), ("scratch", 0x8004), ("out_group", 0x4004), ("out_pair", 0x5004), ("out_all", 0x6004),
                          ("out_ar", 0x7004), ("row_terms", 0x9004)):
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
    data = dataloader.CountDataset(kmers, np.ones((3, 2, 5), dtype=np.uint32), "dna", 2)
    wide = dataloader.CountDataset(kmers, np.ones((17, 2, 5), dtype=np.uint32), "dna", 2)

    def uniform(codes):
        raise AssertionError("the AR function was called")
    for call in (hypothesis.k_sample, hypothesis.agglomerate):
        with pytest.raises(ValueError, match="sharded"):
            call(dataloader.CountDataset(kmers[:1], np.ones((3, 1, 5), dtype=np.uint32), "dna", 2, shard=(0, 2), total_rows=2), vans=[1.0])
        with pytest.raises(ValueError, match="sharded"):
            call(data.deal_by_kmer(0, 2), vans=[1.0])
        with pytest.raises(ValueError, match="at least 2"):
            call(data, [1], vans=[1.0])
        with pytest.raises(ValueError, match="at least 2"):
            call(data, [], vans=[1.0])
        with pytest.raises(ValueError, match="at most 16"):
            call(wide, vans=[1.0])
        with pytest.raises(ValueError, match="at most 16"):
            call(wide, list(range(17)), vans=[1.0])
        with pytest.raises(ValueError, match="repeated"):
            call(data, [0, 2, 0], vans=[1.0])
        with pytest.raises(ValueError, match="the table has 3"):
            call(data, [0, 3], vans=[1.0])
        with pytest.raises(ValueError, match="no model"):
            call(data)
        for kw in (dict(vans=[1.0, 0.0]), dict(vans=[-1.0]), dict(vans=[float("nan")]), dict(ar_func=uniform, h=0.0), dict(ar_func=uniform, h=[1.0, -2.0])):
            with pytest.raises(ValueError, match="> 0"):
                call(data, **kw)
        with pytest.raises(ValueError, match="come together"):
            call(data, ar_func=uniform)
        with pytest.raises(ValueError, match="come together"):
            call(data, h=1.0, vans=[1.0])
        with pytest.raises(ValueError, match="not both"):
            call(data, bear_path="somewhere", ar_func=uniform, h=1.0)
        with pytest.raises(ValueError, match="at most"):
            call(data, vans=np.ones(17))
    with pytest.raises(ValueError, match="model 2"):
        hypothesis.agglomerate(data, vans=[1.0, 2.0], model=2)
    with pytest.raises(ValueError, match="no model"):
        hypothesis.k_sample_from_sequences([["ACGT"], ["ACGA"]], [1])
    with pytest.raises(ValueError, match="> 0"):
        hypothesis.k_sample_from_sequences([["ACGT"], ["ACGA"]], [1], vans=[0.0])
    with pytest.raises(ValueError, match="at most 16"):
        hypothesis.k_sample_from_sequences([["ACGT"]] * 17, [1], vans=[1.0])
    with pytest.raises(ValueError, match="groups of sequences"):
        hypothesis.k_sample_from_sequences([["ACGT"]], [1], vans=[1.0])
    # the result: the entry's pair order into symmetric matrices
    G, M = 3, 2
    pair = np.arange(M * 3 * 2, dtype=np.float64).reshape(M, 3, 2) + 100
    r = hypothesis.KSampleResult(["bear(h=1)", "van(1)"], 1, np.arange(6.0).reshape(M, G), pair, np.array([[7.0, 8.0], [9.0, 10.0]]),
                                 np.array([10.0, 20.0, 30.0]), None)
    assert r.log_bf.shape == r.log_marg_pair.shape == (M, G, G)
    for m in range(M):
        assert np.array_equal(r.log_bf[m], r.log_bf[m].T) and np.array_equal(r.log_marg_pair[m], r.log_marg_pair[m].T)
        assert not np.diag(r.log_bf[m]).view(np.int64).any() and np.array_equal(np.diag(r.log_marg_pair[m]), r.log_marg[m])
        for p, (g, g2) in enumerate(ku.pairs(G)):
            assert r.log_marg_pair[m, g, g2] == pair[m, p, 0] and r.log_bf[m, g2, g] == pair[m, p, 1]
    assert r.log_marg_all.tolist() == [7.0, 9.0] and r.log_bf_all.tolist() == [8.0, 10.0]
    assert r.gof_log_bf().tolist() == [[-10.0, -19.0, -28.0]]
    assert hypothesis.KSampleResult(["van(1)"], 0, np.zeros((1, 2)), np.zeros((1, 1, 2)), np.zeros((1, 2)), None, None).gof_log_bf().shape == (0, 2)


# ------------------------------------------------------------------------------------------- the oracle
def test_oracle_at_two_groups_is_the_two_sample_oracle():
    cols, prior = ku.columns(5, 2)
    a, b, _ = tu.base_rows(5)
    assert np.array_equal(cols[0], a) and np.array_equal(cols[1], b)
    rows = ku.oracle_rows(cols, prior, tu.HS, tu.VANS)
    val, mass, ar, ar_mass = tu.oracle_rows(a, b, prior, tu.HS, tu.VANS)
    for k, (x, y) in enumerate(((val, ar), (mass, ar_mass))):
        assert np.all(rows["group"][k] == x[:, :, :2]) and np.all(rows["pair"][k][:, :, 0, :] == x[:, :, 2:]) and np.all(rows["ar"][k] == y)
        assert np.all(rows["all"][k] == x[:, :, 2:])                           # two groups: all of them are the pair
    sums, want = ku.oracle_sums(rows), tu.oracle_sums((val, mass, ar, ar_mass))
    assert np.array_equal(sums["pair"][0][:, 0], want[0][:, 2:]) and np.array_equal(sums["ar"][1], want[3])
    idx = tu.table_index(len(a), 300, seed=3)
    assert np.array_equal(ku.oracle_sums(rows, idx)["group"][0], tu.oracle_sums((val, mass, ar, ar_mass), idx)[0][:, :2])


@pytest.mark.parametrize("W,G", [(5, 16), (21, 3)])
def test_oracle_rows_of_every_kind_and_its_scipy_twin(W, G):
    cols, prior = ku.columns(W, G)
    hs, vans = (tu.HS, tu.VANS) if W == 5 else (tu.HS[1:2], tu.VANS[1:2])
    rows = ku.oracle_rows(cols, prior, hs, vans)
    n = cols.astype(np.uint64).sum(2)                                             # [G, N]
    if G >= 4:
        assert not cols[-1].any() and all(v == 0 for v in rows["group"][0][:, :, -1].reshape(-1))
    assert (cols.astype(np.uint64).sum(0) >= 2 ** 33 - 2).any() and (n.sum(0) > 2 ** 35).any()      # pooled beyond a 32-bit cell
    nonempty = (n > 0).sum(0)
    assert (nonempty >= 3).any() and (G > 4 or (nonempty == 1).any())            # (sixteen rotated columns leave no row to one group)
    for p, (g, g2) in enumerate(ku.pairs(G)):                                     # exact zeros, at 50 digits
        one_side = (n[g] == 0) | (n[g2] == 0)
        assert one_side.any() and all(v == 0 for v in rows["pair"][0][one_side][:, :, p, 1].reshape(-1))
        if not (G >= 4 and g2 == G - 1):               # (a bracket of two non-empty sides CAN be zero: (1, 0, ..) and (1, 1, ..) under van = 1)
            assert (~one_side).any() and any(v != 0 for v in rows["pair"][0][~one_side][:, :, p, 1].reshape(-1))
    assert all(v == 0 for v in rows["all"][0][nonempty <= 1][:, :, 1].reshape(-1))
    sums = ku.oracle_sums(rows)
    ok = cols.astype(np.uint64).max((0, 2)) < 2 ** 31 // G                        # (float64 gammaln cancels at the counter's limit)
    twin = ku.scipy_sums(cols[:, ok], prior[ok], hs, vans)
    part = ku.oracle_sums(rows, np.flatnonzero(ok))
    for key, got in zip(ku.KEYS, twin):
        want, mass = part[key]
        assert got.shape == want.shape and np.all(np.abs(got - want) <= 1e-9 * mass + 1e-300), key
        assert np.all(sums[key][1] >= np.abs(sums[key][0]))


# ------------------------------------------------------------------------------------------- the statistical case and the merge loop
@pytest.mark.parametrize("alphabet", ["dna", "prot"])
def test_merge_loop_on_the_statistical_case(alphabet):
    """Six groups of 100 sequences x 120 letters, alternately from two chains (ku.GROUPS); van = 1 and uniform AR rows with h = 0.05
    and 5.  Under every lag and model: every same-source pair has log_bf <= -46, every cross pair >= +147, the greedy loop ends at
    the two sources with the smallest remaining Bayes factor above +1000, and the three groups of the first source alone have
    log_bf_all <= -99.  (log_bf_all of all six is negative at the higher lags -- six distributions overfit where two would do -- so
    no sign is asserted for it: the partition is the test.)"""
    from bear_amd import hypothesis
    W = len(tu.LETTERS[alphabet]) + 1
    seqs = ku.stat_sequences(alphabet)
    same = [(g, g2) for g, g2 in ku.pairs(6) if (g - g2) % 2 == 0]
    for lag in tu.STAT_CASE[alphabet][1]:
        cols = ku.count_host(seqs, lag, alphabet)
        assert cols.shape[0] == 6 and cols.shape[2] == W and np.all(cols.sum((1, 2)) == 100 * 121)
        prior = np.full(cols.shape[1:], 1.0 / W)
        _, pair, both, _ = ku.scipy_sums(cols, prior, ku.STAT_HS, ku.STAT_VANS)
        _, _, p1, _ = ku.scipy_sums(cols[0::2], prior, ku.STAT_HS, ku.STAT_VANS)
        for m in range(3):
            bf = {pr: pair[m, p, 1] for p, pr in enumerate(ku.pairs(6))}
            print(f"{alphabet} lag {lag} model {m}: same source max {max(bf[p] for p in same):.1f}, cross min "
                  f"{min(v for p, v in bf.items() if p not in same):.1f}, all six {both[m, 1]:.1f}, the first source's three {p1[m, 1]:.1f}")
            assert all(bf[p] <= -46 for p in same) and all(v >= 147 for p, v in bf.items() if p not in same)
            assert p1[m, 1] <= -99
            res = hypothesis.merge_loop(list(cols), range(6), ku.scipy_evaluate(m), lambda a, b: a + b)
            assert res.partition == ku.PARTITION and len(res.merges) == 4 and res.log_evidence.shape == (5,)
            assert all(x < 0 for _, _, x in res.merges)
            assert all((set(a) | set(b)) <= set(ku.PARTITION[0]) or (set(a) | set(b)) <= set(ku.PARTITION[1]) for a, b, _ in res.merges)
            gains = np.diff(res.log_evidence)
            assert np.allclose(gains, [-x for _, _, x in res.merges], rtol=1e-9, atol=1e-6)
            final = ku.scipy_evaluate(m)([cols[0::2].sum(0, dtype=np.uint32), cols[1::2].sum(0, dtype=np.uint32)])[1][0, 1]
            assert final > 1000


def test_merge_loop_ties_stops_and_single_cluster():
    """The loop alone, on made-up evidence: ties go to the lower (g, g'), nothing is merged at log_bf >= 0, and clusters that all
    attract each other end as one."""
    from bear_amd import hypothesis

    def evaluate_from(bf_of):
        def evaluate(tables):
            K = len(tables)
            bf = np.zeros((K, K))
            for g in range(K):
                for g2 in range(g + 1, K):
                    bf[g, g2] = bf[g2, g] = bf_of(tables[g], tables[g2])
            return np.array([float(len(t)) for t in tables]), bf
        return evaluate
    pool = lambda a, b: a + b                                                      # a table here is the list of its members
    res = hypothesis.merge_loop([[0], [1], [2], [3]], [10, 11, 12, 13], evaluate_from(lambda a, b: -1.0), pool)
    assert res.partition == [[10, 11, 12, 13]] and [m[:2] for m in res.merges] == [([10], [11]), ([10, 11], [12]), ([10, 11, 12], [13])]
    assert res.log_evidence.tolist() == [4.0] * 4
    res = hypothesis.merge_loop([[0], [1], [2]], [0, 1, 2], evaluate_from(lambda a, b: 0.0), pool)
    assert res.partition == [[0], [1], [2]] and res.merges == [] and res.log_evidence.tolist() == [3.0]
    res = hypothesis.merge_loop([[0], [1], [2], [3]], range(4), evaluate_from(lambda a, b: -2.0 if (a[0] + b[0]) % 2 == 0 else 5.0), pool)
    assert res.partition == [[0, 2], [1, 3]] and [m[:2] for m in res.merges] == [([0], [2]), ([1], [3])]
