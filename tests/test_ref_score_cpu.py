"""CPU tests of bear_ref models downstream of training (kernels_refscore.h, gen_run<.., REF> of kernels_generate.h,
bear_ref_prior_rows_f64, bear_generate_whole_ref_f64; get_var_probs.RefModel): a NumPy replica of the reference-mixed prior row
with an exact fma, held to the oracle's ``ref_ar_func`` and to ``bear_ref._make_ref_ar_func``'s torch ops; the generation cases of
the GPU file under that replica, each decided by a margin; and the two entries in the header and the binding.
``tests/test_ref_score_gpu.py`` compares the kernels' bits and bytes with what is computed here."""
import ctypes
import fractions
import functools
import math

import numpy as np
import pytest

import bear_oracle as o
import test_generate_cpu as g
import test_generate_whole_cpu as w
from util import abi_header

EPS = o.EPSILON
RTOL = 1e-14                         # what tests/test_ref_mix_gpu.py holds the training forward to against o.ref_ar_func
MAX_LEN = w.MAX_LEN                  # 48
N_SEQS = (37, 65)


# ------------------------------------------------------------------------------------------- the replica
if hasattr(math, "fma"):
    _fma1 = math.fma
else:
    def _fma1(a, b, c):
        """a * b + c rounded once: the exact rational, then float()'s correctly rounded conversion."""
        return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.fromiter((_fma1(x, y, z) for x, y, z in zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())),
                      dtype=np.float64, count=a.size)
    return out.reshape(a.shape)


def ref_total(r):
    """R of rows r [n, W] (stop entry zero) in rfw_ref_total's order: below 8 entries one after the other; else eight running
    sums over the whole blocks of eight, combined pairwise, then the rest -- the order of NumPy's add.reduce
    (test_ref_total_is_numpys_order)."""
    W = r.shape[1]
    if W < 8:
        s = r[:, 0].copy()
        for b in range(1, W - 1):
            s = s + r[:, b]
        return s
    full = W - W % 8
    q = [r[:, j].copy() for j in range(8)]
    for i in range(8, full, 8):
        for j in range(8):
            q[j] = q[j] + r[:, i + j]
    s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))
    for i in range(full, W - 1):
        s = s + r[:, i]
    return s


def mix_rows(ref_rows, g_rows, tau, nw, eps=EPS):
    """prior [n, W] of reference count rows [n, W] (uint32 values) and net rows ``g_rows`` [n, W] (None: the one-hot at the
    stop): the formula of include/bear_hip.h, operation by operation.  E = exp(-tau) is ``math.exp``, the C library's, as the
    entry forms it."""
    ref_rows = np.asarray(ref_rows)
    n, W = ref_rows.shape
    A = W - 1
    E, V = math.exp(-tau), 1.0 / (nw + 1.0)
    r = ref_rows.astype(np.float64) + eps
    r[:, -1] = 0.0
    R = ref_total(r)
    dev = r / R[:, None] - 1.0 / A
    dev[:, -1] = 0.0
    shape = np.r_[np.full(A, 1.0 / A), 0.0]
    if g_rows is None:
        g_rows = np.zeros((n, W))
        g_rows[:, -1] = 1.0
    jc = fma(E, dev, shape[None, :])
    return fma(nw, g_rows, jc) * V + eps


def ref_rows_of(keys, ref_table, ref_counts):
    """The reference count rows [n, W] (uint32 values as int64) of keys: searchsorted in the ascending table, zeros where absent."""
    keys = np.asarray(keys, dtype=np.uint64)
    rows = np.zeros((keys.size, ref_counts.shape[1]), dtype=np.int64)
    if ref_table.size:
        pos = np.minimum(np.searchsorted(ref_table, keys), ref_table.size - 1)
        found = ref_table[pos] == keys
        rows[found] = ref_counts[pos[found]].astype(np.int64) & 0xFFFFFFFF
    return rows


def ref_rows_replica(keys, ref_table, ref_counts, g, tau, nw):
    """The NumPy replica of bear_ref_prior_rows_f64: prior [n, W] of the query ``keys`` (uint64, any order).  ``ref_table`` uint64 [N]
    ascending, ``ref_counts`` [N, W] (uint32 in int32 storage); ``g``: None (the stop net function), rows [n, W], or a function
    keys -> rows."""
    keys = np.asarray(keys, dtype=np.uint64)
    return mix_rows(ref_rows_of(keys, ref_table, ref_counts), g(keys) if callable(g) else g, tau, nw)


def per_distinct_key(rows_of_keys):
    """``rows_of_keys`` asked once per distinct key (a row is a pure function of its key; the exact fma is slow)."""
    memo = {}

    def rows(keys):
        keys = np.asarray(keys, dtype=np.uint64)
        new = np.array(sorted(set(keys.tolist()) - set(memo)), dtype=np.uint64)
        if new.size:
            memo.update(zip(new.tolist(), rows_of_keys(new)))
        return np.stack([memo[k] for k in keys.tolist()])
    rows.memo = memo
    return rows


# ------------------------------------------------------------------------------------------- the rows the checks run on
def special_rows(W, rng):
    """Reference rows [n, W] (uint32 values): a flat all-zero row, a single huge count (4e9: beyond int32), rows with a non-zero
    stop count next to their twins without it, small and large random rows."""
    rows = [np.zeros(W, dtype=np.int64)]
    huge = np.zeros(W, dtype=np.int64)
    huge[1] = 4_000_000_000
    rows.append(huge)
    for _ in range(6):
        a = rng.integers(0, 50, size=W)
        b = a.copy()
        a[-1], b[-1] = 0, rng.integers(1, 1000)
        rows += [a, b]
    rows += list(rng.integers(0, 2 ** 32, size=(8, W)))
    rows += list(rng.integers(0, 3, size=(8, W)))
    return np.array(rows, dtype=np.int64)


MODELS = ((1 / 30, 0.01), (0.7, 2.5), (0.2, 0.3))     # (tau, nw): bear_ref's initial values, and two a training run may reach


@pytest.mark.parametrize("W", [5, 21])
def test_ref_total_is_numpys_order(W):
    rng = np.random.default_rng(W)
    r = special_rows(W, rng).astype(np.float64) + EPS
    r[:, -1] = 0.0
    assert np.array_equal(ref_total(r), np.add.reduce(r, axis=-1)) and np.array_equal(ref_total(r), np.abs(r).sum(-1))


def test_fma_rounds_once():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    assert fma(a, b, -1.0) == -2.0 ** -60 and a * b - 1.0 == 0.0
    assert np.array_equal(fma(np.array([3.0, 0.1]), 2.0, np.array([[1.0], [0.5]])), np.array([[7.0, 0.1 * 2 + 1.0], [6.5, 0.7]]))


@pytest.mark.parametrize("W", [5, 21])
@pytest.mark.parametrize("net", ["stop", "rows"])
def test_replica_against_the_oracle_and_the_torch_ops(W, net):
    """``ref_rows_replica`` against ``oracle.ref_ar_func(g, oracle.ref_input(rows), log tau, log nw) + eps`` and against
    ``bear_ref._make_ref_ar_func``'s torch ops on the CPU, both at RTOL; a stop count in the reference row does not matter."""
    import torch
    from bear_amd import bear_ref
    rng = np.random.default_rng(100 + W)
    rows = special_rows(W, rng)
    n = rows.shape[0]
    table = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    counts = rows.astype(np.uint32).view(np.int32)
    assert (counts < 0).any()                                           # uint32 in int32 storage
    order = rng.permutation(n)
    keys = np.concatenate([table[order], [np.uint64(0), np.uint64(5)]])   # unsorted, with two absent keys
    want_rows = np.concatenate([rows[order], np.zeros((2, W), dtype=np.int64)])
    g_rows = rng.dirichlet(np.full(W, 0.5), size=keys.size) if net == "rows" else None
    one_hot = np.zeros((keys.size, W))
    one_hot[:, -1] = 1.0
    for tau, nw in MODELS:
        got = ref_rows_replica(keys, table, counts, g_rows, tau, nw)
        want = o.ref_ar_func(one_hot if g_rows is None else g_rows, o.ref_input(want_rows), np.log(tau), np.log(nw)) + EPS
        err = np.abs(got - want) / np.abs(want)
        print(f"W {W} net {net} tau {tau:.3g} nw {nw:.3g}: largest relative difference to the oracle {err.max():.2e}")
        assert np.allclose(got, want, rtol=RTOL, atol=0)
        g_t = torch.from_numpy(one_hot if g_rows is None else g_rows)
        ar_func, params = bear_ref._make_ref_ar_func(3, W - 1, lambda lag, A, dtype, device: ((lambda codes: g_t), []), {},
                                                     device=torch.device("cpu"))
        with torch.no_grad():
            params[0].fill_(float(np.log(tau)))
            params[1].fill_(float(np.log(nw)))
            torch_rows = (ar_func(None, bear_ref._ref_input(torch.from_numpy(want_rows.astype(np.uint32).view(np.int32)))) + EPS).numpy()
        assert np.allclose(got, torch_rows, rtol=RTOL, atol=0)
        assert got.min() > 0 and np.allclose(got.sum(1), 1.0 + W * EPS, rtol=1e-12)
    # the twins with and without a stop count give the same bits; an absent key is the all-zero row
    twins = ref_rows_replica(table[2:14], table, counts, None, 0.2, 0.3)
    assert np.array_equal(twins[0::2], twins[1::2])
    assert np.array_equal(ref_rows_replica(np.array([5], dtype=np.uint64), table, counts, None, 0.2, 0.3),
                          ref_rows_replica(table[:1], table, counts, None, 0.2, 0.3))


# ------------------------------------------------------------------------------------------- the generation cases both files run
# (alphabet, lag, net function, model): h, tau, nw per case
REF_CASES = [("dna", 1, "stop", "bear"), ("dna", 21, "stop", "bear"), ("prot", 5, "stop", "bear"), ("prot", 12, "stop", "ar_map"),
             ("prot", 5, "lin", "bear")]
REF_CASE_IDS = ["-".join(map(str, c)) for c in REF_CASES]
CASE_SCALARS = {"bear": dict(h=0.25, tau=0.2, nw=0.3), "ar_map": dict(tau=1 / 30, nw=0.02)}
CASE_SEEDS = {c: 7100 + 10 * i for i, c in enumerate(REF_CASES)}


@functools.lru_cache(maxsize=None)
def ref_case_inputs(case):
    """``inputs`` of a case: the train table and the reference table -- counted from OTHER strings, four of the twelve shared, so
    there are k-mers in one table, the other and both (and a generated sequence leaves both) -- the model's scalars, ``mat`` of a
    linear case."""
    name, lag, net, model = case
    W, rank, seed = len(g.ALPHABETS[name]) + 1, g.ranks(name), CASE_SEEDS[case]
    rng = np.random.default_rng(seed)
    strings = [rng.integers(0, W - 1, size=int(rng.integers(6, 31))) for _ in range(12)]
    table, counts = w.count_symbols(strings[:8] + [np.zeros(0, dtype=np.int64)], rank, lag, times=3)      # (an empty string: a stop count at the start)
    ref_table, ref_counts = w.count_symbols(strings[4:], rank, lag, times=2)
    mat = rng.normal(size=(lag, 21, 21)) * 0.5 if net == "lin" else None
    sample = np.arange(max(N_SEQS), dtype=np.uint64) * np.uint64(3) + np.uint64(7)
    inputs = dict(table=table, counts=counts, ref_table=ref_table, ref_counts=ref_counts, sample=sample, seed=seed, W=W, rank=rank,
                  lag=lag, mat=mat, **CASE_SCALARS[model])
    for a in inputs.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inputs


def case_prior(case):
    """The replica's AR function of a case, keys -> [n, W] (asked once per distinct key), and the keys it was asked for."""
    inputs = ref_case_inputs(case)
    net = functools.partial(w.linear_rows, mat=inputs["mat"], rank=inputs["rank"], lag=inputs["lag"]) if inputs["mat"] is not None else None
    return per_distinct_key(functools.partial(ref_rows_replica, ref_table=inputs["ref_table"], ref_counts=inputs["ref_counts"], g=net,
                                              tau=inputs["tau"], nw=inputs["nw"]))


def run_ref_replica(case, n_steps=MAX_LEN, n_seq=max(N_SEQS), sample=None):
    inputs = ref_case_inputs(case)
    sample = inputs["sample"][:n_seq] if sample is None else sample
    prior = case_prior(case)
    letters = np.full((n_seq, n_steps), 0xFF, dtype=np.uint8)
    kw = dict(h=inputs["h"]) if "h" in inputs else dict(get_map=True)
    keys, left, length, stopped, gap = w.replica_whole(inputs["table"], inputs["counts"], inputs["rank"], inputs["lag"],
                                                       w.start_keys(n_seq, inputs["rank"], inputs["lag"]), sample, np.full(n_seq, n_steps),
                                                       np.zeros(n_seq), np.zeros(n_seq), 0, n_steps, inputs["seed"], prior=prior,
                                                       letters=letters, **kw)
    return dict(letters=letters, keys=keys, left=left, length=length, stopped=stopped, gap=gap,
                visited=np.array(sorted(prior.memo), dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def ref_expected(case, n_seq=max(N_SEQS)):
    """The replica's answer for a case, computed once for the 65 sequences and left unchanged; sequences are independent, so the
    first 37 are the answer for 37 (the gap is the smallest of all 65)."""
    if n_seq != max(N_SEQS):
        full = ref_expected(case)
        return {k: (v[:n_seq] if isinstance(v, np.ndarray) and k != "visited" else v) for k, v in full.items()}
    out = run_ref_replica(case)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("case", REF_CASES, ids=REF_CASE_IDS)
def test_gpu_cases_are_decided_by_a_margin(case):
    """Every draw of every case the GPU test runs is decided by more than MIN_GAP, so the kernel's bytes must EQUAL the replica's."""
    want = ref_expected(case)
    n = max(N_SEQS)
    print(case, "smallest gap", want["gap"], "stopped", int(want["stopped"].sum()), "of", n, "zero lengths", int((want["length"] == 0).sum()),
          "cut", int((want["stopped"] == 0).sum()), "distinct k-mers", want["visited"].size)
    assert want["gap"] > g.MIN_GAP
    W = ref_case_inputs(case)["W"]
    for i in range(n):
        m = want["length"][i]
        assert np.all(want["letters"][i, :m] < W - 1) and np.all(want["letters"][i, m:] == 0xFF)
        assert want["left"][i] == (0 if want["stopped"][i] else MAX_LEN - m) and (want["stopped"][i] or m == MAX_LEN)
    for n_seq in N_SEQS:
        part = ref_expected(case, n_seq)
        assert part["letters"].shape == (n_seq, MAX_LEN) and part["keys"].shape == (n_seq,)


def test_cases_stop_are_cut_and_stop_at_once():
    """Across the cases some sequences stop, some are cut at MAX_LEN, and some draw the stop first (length 0)."""
    stopped = np.concatenate([ref_expected(c)["stopped"] for c in REF_CASES]).astype(bool)
    length = np.concatenate([ref_expected(c)["length"] for c in REF_CASES])
    assert stopped.any() and (~stopped).any() and np.all(length[~stopped] == MAX_LEN)
    assert np.any(stopped & (length == 0)) and np.any(stopped & (length > 0))


def test_cases_meet_kmers_of_one_table_the_other_both_and_neither():
    seen = set()
    for case in REF_CASES:
        inputs, want = ref_case_inputs(case), ref_expected(case)
        in_train, in_ref = np.isin(want["visited"], inputs["table"]), np.isin(want["visited"], inputs["ref_table"])
        seen |= set(zip(in_train.tolist(), in_ref.tolist()))
        if inputs["lag"] == 1:          # (five contexts in all: both tables hold every one)
            continue
        assert np.setdiff1d(inputs["table"], inputs["ref_table"]).size and np.setdiff1d(inputs["ref_table"], inputs["table"]).size
        assert np.intersect1d(inputs["table"], inputs["ref_table"]).size
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


def test_the_reference_row_moves_the_letters():
    """The same case without its reference table (every k-mer absent: the flat row) writes other letters: the mixing is not idle."""
    case = REF_CASES[2]
    inputs, want = ref_case_inputs(case), ref_expected(case, 37)
    flat = per_distinct_key(functools.partial(ref_rows_replica, ref_table=np.zeros(0, dtype=np.uint64),
                                              ref_counts=np.zeros((0, inputs["W"]), dtype=np.int32), g=None, tau=inputs["tau"], nw=inputs["nw"]))
    letters = np.full((37, MAX_LEN), 0xFF, dtype=np.uint8)
    w.replica_whole(inputs["table"], inputs["counts"], inputs["rank"], inputs["lag"], w.start_keys(37, inputs["rank"], inputs["lag"]),
                    inputs["sample"][:37], np.full(37, MAX_LEN), np.zeros(37), np.zeros(37), 0, MAX_LEN, inputs["seed"], prior=flat,
                    h=inputs["h"], letters=letters)
    assert not np.array_equal(letters, want["letters"])


# ------------------------------------------------------------------------------------------- header and binding
def test_entries_declared_bound_and_refusing():
    """The header declares both entries, the binding holds them, the ABI version stays 12, and every refusal of the header comes
    before any device call (this test runs without a device)."""
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    assert version == 12 == _lib.ABI_VERSION
    vp, i, u64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_double
    want_rows = [vp, vp, u64, i, vp, u64, vp, d, d, d, vp, vp]
    whole = sigs["bear_generate_whole_f64"][1]
    want_gen = whole[:-1] + [vp, vp, u64, d, d, d, i, vp]            # bear_generate_whole_f64's, then the reference column and the model
    for name, want in (("bear_ref_prior_rows_f64", want_rows), ("bear_generate_whole_ref_f64", want_gen)):
        assert name in _lib.SYMBOLS and sigs[name] == (i, want)
        fn = getattr(_lib.lib(), name)
        assert fn.restype is i and list(fn.argtypes) == want
    assert callable(kernels.ref_prior_rows) and callable(kernels.generate_whole_ref)
    assert (kernels.GEN_NET_STOP, kernels.GEN_NET_ROWS, kernels.GEN_NET_MAT) == (0, 1, 2)
    fake, odd = ctypes.c_void_p(8), ctypes.c_void_p(10)      # pointers that are "given": never dereferenced, every refusal comes first
    nan, inf = float("nan"), float("inf")

    rows = _lib.lib().bear_ref_prior_rows_f64

    def call_rows(width=5, n_ref=0, ref=(None, None), n_query=0, query=None, net_rows=None, tau=0.2, nw=0.3, eps=1e-7, prior=None):
        return rows(*ref, n_ref, width, query, n_query, net_rows, tau, nw, eps, prior, None)
    assert call_rows() == 0 and call_rows(width=21) == 0 and call_rows(n_ref=3, ref=(fake, fake)) == 0      # n_query = 0, n_ref = 0: valid
    assert call_rows(width=4) == -1 and call_rows(width=20) == -1
    for bad in (0.0, -1.0, nan, inf):
        assert call_rows(tau=bad) == -1 and call_rows(nw=bad) == -1
    assert call_rows(eps=nan) == -1 and call_rows(eps=-1e-7) == -1 and call_rows(eps=0.0) == 0
    assert call_rows(n_ref=2 ** 32 - 1, ref=(fake, fake)) == -1
    assert call_rows(n_ref=1, ref=(None, fake)) == -1 and call_rows(n_ref=1, ref=(fake, None)) == -1 and call_rows(n_ref=1, ref=(odd, fake)) == -1
    assert call_rows(n_query=1, query=None, prior=fake) == -1 and call_rows(n_query=1, query=fake, prior=None) == -1
    assert call_rows(n_query=1, query=odd, prior=fake) == -1 and call_rows(n_query=1, query=fake, prior=odd) == -1
    assert call_rows(n_query=1, query=fake, prior=fake, net_rows=odd) == -1

    gen = _lib.lib().bear_generate_whole_ref_f64
    dna, prot = kernels.score_ranks("dna").ctypes.data, kernels.score_ranks("prot").ctypes.data

    def call(lag=3, width=5, rank=dna, mode=1, get_map=0, h=1.0, prior=None, mat=None, step0=0, n_steps=4, stride=4, n_seq=0,
             state=(None, None, None, None, None), letters=None, n_ref=0, ref=(None, None), tau=0.2, nw=0.3, eps=1e-7, net=0):
        return gen(None, None, 0, lag, width, rank, mode, get_map, h, 0.0, prior, mat, 1, *state, n_seq, step0, n_steps, letters, stride,
                   None, *ref, n_ref, tau, nw, eps, net, None)
    wide = dict(width=21, rank=prot)
    assert call() == 0 and call(lag=21) == 0 and call(lag=12, **wide) == 0 and call(mode=2, get_map=1) == 0
    assert call(net=1, prior=fake, n_steps=1) == 0 and call(net=2, mat=fake, n_steps=40, stride=40, **wide) == 0
    assert call(mode=0) == -1 and call(mode=3) == -1                       # a BMM has nothing to mix
    assert call(mode=2, get_map=0) == -1 and call(h=0.0) == -1 and call(h=nan) == -1
    assert call(net=3) == -1 and call(net=-1) == -1
    assert call(net=0, prior=fake, n_steps=1) == -1 and call(net=0, mat=fake, **wide) == -1        # rows against `net`
    assert call(net=1) == -1 and call(net=1, mat=fake, **wide) == -1 and call(net=2, **wide) == -1 and call(net=2, prior=fake, n_steps=1, **wide) == -1
    assert call(net=1, prior=fake, n_steps=2) == -1                        # more than one step with rows
    assert call(net=2, mat=fake) == -1                                     # mat at width 5
    assert call(width=4) == -1 and call(lag=0) == -1 and call(lag=22) == -1 and call(lag=13, **wide) == -1
    assert call(step0=3, n_steps=2, stride=4) == -1 and call(step0=3, n_steps=1, stride=4) == 0
    for bad in (0.0, -1.0, nan, inf):
        assert call(tau=bad) == -1 and call(nw=bad) == -1
    assert call(eps=nan) == -1 and call(n_ref=2 ** 32 - 1) == -1
    ok = (fake,) * 5
    for state in ((fake, fake, fake, None, fake), (fake, fake, fake, fake, None), (fake, fake, fake, odd, fake), (None, fake, fake, fake, fake)):
        assert call(n_seq=1, state=state, letters=fake) == -1, state
    assert call(n_seq=1, state=ok, letters=fake, n_ref=1, ref=(None, fake)) == -1
    assert call(n_seq=1, state=ok, letters=fake, n_ref=1, ref=(fake, None)) == -1
    assert call(n_seq=1, state=ok, letters=fake, n_ref=1, ref=(odd, fake)) == -1
    assert call(n_seq=1, net=2, mat=odd, state=ok, letters=fake, **wide) == -1
