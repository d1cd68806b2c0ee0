"""CPU tests of sequence generation on the device (kernels_generate.h, bear_generate_steps_f64): a NumPy replica of the kernel's rule
on the oracle's counter streams, what the rule promises (a sequence that returns to a k-mer meets the same table row; the first
letter follows the posterior mean), the margin that lets the GPU comparison be exact, and the entry in the header and the binding.

The replica is built from ``bear_oracle.log_gamma_keys`` (the log-Gamma draw), ``_cell_key`` and ``_mix64`` (the keys); restated
here are only the Gumbel transform and the key shift.  ``tests/test_generate_gpu.py`` compares the kernel's letters with it."""
import ctypes
import functools

import numpy as np
import pytest
from scipy import stats as st

import bear_oracle as o
from util import abi_header

GEN_ID_GUMBEL = 3000
BITS = {5: 3, 21: 5}
MAX_LAG = {5: 21, 21: 12}
ALPHABETS = {"dna": "ACGT", "prot": "ARNDCEQGHILKMFPSTWYV"}
Z_MAX = st.norm.ppf(0.9995)          # the project's criterion (test_tie_noise_gpu.py), here on a standardised frequency
MIN_GAP = 1e-6                       # best minus second-best score: draws agree to ~1e-13 relative between host and device
                                     # (DRAW_RTOL of test_sampling_gpu.py) and scores are O(100), so such a gap cannot flip


def ranks(alphabet_name):
    """kernels.score_ranks restated: rank[c] = position of letter c among the letters and '[' in byte order; 0xFF for the stop."""
    letters = ALPHABETS[alphabet_name]
    order = sorted(letters + "[")
    W = len(letters) + 1
    rank = np.full(W + 1, 0xFF, dtype=np.uint8)
    for c, ch in enumerate(letters):
        rank[c] = order.index(ch)
    rank[W] = order.index("[")
    return rank


def pack(codes, rank, W):
    """Keys uint64 [n] of letter codes [n, lag]: ranks, first letter most significant."""
    keys = np.zeros(codes.shape[0], dtype=np.uint64)
    for p in range(codes.shape[1]):
        keys = (keys << np.uint64(BITS[W])) | rank[codes[:, p]].astype(np.uint64)
    return keys


def unpack_codes(keys, rank, W, lag):
    """core.encode_kmers codes int8 [n, lag] of keys: letters 0 .. W - 2, '[' = W - 1."""
    code_of_rank = np.zeros(1 << BITS[W], dtype=np.int8)
    code_of_rank[rank[:W - 1]] = np.arange(W - 1)
    code_of_rank[rank[W]] = W - 1
    shifts = (np.arange(lag - 1, -1, -1) * BITS[W]).astype(np.uint64)
    return code_of_rank[((keys[:, None] >> shifts[None, :]) & np.uint64((1 << BITS[W]) - 1)).astype(np.int64)]


def prior_rows(keys, W):
    """A stand-in AR function for the stepwise cases: rows [n, W] > 0.02 that sum to 1, a pure function of the end key."""
    cell = keys[:, None] * np.uint64(W) + np.arange(W, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        f = 0.05 + o._u01(o._mix64(cell ^ np.uint64(0xA5A5A5A5)))
    return f / f.sum(axis=1, keepdims=True)


def replica(table, counts, rank, lag, keys, sample, left, step0, n_steps, seed, van=None, prior=None, h=None, get_map=False,
            letters=None, trace=None):
    """The rule of generate_steps_kernel.  ``table`` uint64 ascending, ``counts`` [N, W]; ``keys`` / ``left`` are returned updated
    (the inputs are left alone); ``prior``: None or a function keys -> [n, W] (it is asked once per step, as the host loop asks an AR
    function); ``letters`` uint8 [n, L] is filled in place.  Returns ``(keys, left, smallest best-minus-second-best score)``;
    ``trace``, a list, receives ``(step, sequence indices, keys, table values)`` per step."""
    W = rank.size - 1
    bits, mask = np.uint64(BITS[W]), np.uint64((1 << (BITS[W] * lag)) - 1)
    keys, left = np.array(keys, dtype=np.uint64), np.array(left, dtype=np.int64)
    sample = np.asarray(sample, dtype=np.uint64)
    b = np.arange(W - 1, dtype=np.uint64)[None, :]
    gap = np.inf
    for k in range(n_steps):
        live = np.flatnonzero(left > 0)
        if live.size == 0:
            break
        t, q, s = step0 + k, keys[live], sample[live][:, None]
        c = np.zeros((live.size, W - 1))
        if table.size:
            pos = np.minimum(np.searchsorted(table, q), table.size - 1)
            found = table[pos] == q
            c[found] = counts[pos[found], :W - 1]
        if prior is None:
            conc = van + c
        elif h is None:
            conc = prior(q)[:, :W - 1]
        else:
            conc = prior(q)[:, :W - 1] * (1.0 / h) + c
        with np.errstate(over="ignore"):
            if get_map:
                tv = np.log(conc)
            else:
                tkey = o._cell_key(seed, 0, s, o._mix64(q)[:, None] + b)
                tv = o.log_gamma_keys(conc.reshape(-1), tkey.reshape(-1)).reshape(conc.shape)
            gumbel = -np.log(-np.log(o._u01(o._cell_key(seed, GEN_ID_GUMBEL, s, np.uint64(t * W) + b))))
        score = tv + gumbel
        best = np.argmax(score, axis=1)                        # the lowest letter with the largest score
        top = np.sort(score, axis=1)
        gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
        if trace is not None:
            trace.append((t, live, q, tv))
        with np.errstate(over="ignore"):
            keys[live] = ((q << bits) | rank[best].astype(np.uint64)) & mask
        letters[live, t] = best
        left[live] -= 1
    return keys, left, gap


# ------------------------------------------------------------------------------------------- the cases both test files run
N_SEQ = 37
LENGTHS = (np.arange(N_SEQ) * 17 + 5) % 41        # 37 unequal lengths 0 .. 40, with a 0 and a 40 among them
TABLES = ("trained", "one_key", "empty")
MODELS = ("bmm", "bmm_map", "bear", "ar_map")


def make_table(alphabet_name, lag, kind, seed):
    """``(table uint64 [N] ascending, counts int32 [N, W], seed end keys uint64 [N_SEQ])``.  'trained': the transitions of a few
    random strings, counted three times over, with the seeds cut from those strings -- a sequence follows them for a while (rows
    that are found, k-mers met again at short lags) and leaves them sooner or later (k-mers the table lacks; at lag 1 none)."""
    W = len(ALPHABETS[alphabet_name]) + 1
    rank = ranks(alphabet_name)
    rng = np.random.default_rng(seed)
    train = rng.integers(0, W - 1, size=(6, 48 + lag))
    windows = np.concatenate([np.lib.stride_tricks.sliding_window_view(row, lag + 1) for row in train])
    ctx = pack(windows[:, :lag], rank, W)
    starts = ctx[rng.integers(0, ctx.size, size=N_SEQ)]
    if kind == "empty":
        return np.zeros(0, dtype=np.uint64), np.zeros((0, W), dtype=np.int32), starts
    table, inverse = np.unique(ctx, return_inverse=True)
    counts = np.zeros((table.size, W), dtype=np.int32)
    np.add.at(counts, (inverse.reshape(-1), windows[:, lag]), 3)
    if kind == "one_key":
        j = int(np.searchsorted(table, starts[0]))
        table, counts = table[j:j + 1], counts[j:j + 1]
    return table, counts, starts


def cases():
    out = []
    for alphabet_name in ("dna", "prot"):
        W = len(ALPHABETS[alphabet_name]) + 1
        for lag in (1, 5, MAX_LAG[W]):
            for model in MODELS:
                out.append((alphabet_name, lag, model, "trained"))
        out += [(alphabet_name, 5, "bmm", "one_key"), (alphabet_name, 5, "bmm", "empty"), (alphabet_name, 5, "bear", "empty")]
    return out


CASES = cases()
CASE_IDS = ["-".join(map(str, c)) for c in CASES]


def model_args(model, W):
    """The keyword arguments a case's model hands the replica and ``kernels.generate_steps`` alike (prior: the function)."""
    if model == "bmm":
        return dict(van=0.5)
    if model == "bmm_map":
        return dict(van=0.5, get_map=True)
    if model == "bear":
        return dict(prior=functools.partial(prior_rows, W=W), h=0.25)
    return dict(prior=functools.partial(prior_rows, W=W), get_map=True)


@functools.lru_cache(maxsize=None)
def expected(case):
    """The replica's answer for a case, computed once: ``(inputs, letters, final keys, final left, smallest gap)``."""
    alphabet_name, lag, model, kind = case
    W = len(ALPHABETS[alphabet_name]) + 1
    seed = 1000 + CASES.index(case)
    table, counts, starts = make_table(alphabet_name, lag, kind, seed)
    sample = np.arange(N_SEQ, dtype=np.uint64) * np.uint64(3) + np.uint64(7)
    letters = np.full((N_SEQ, int(LENGTHS.max())), 0xFF, dtype=np.uint8)
    keys, left, gap = replica(table, counts, ranks(alphabet_name), lag, starts, sample, LENGTHS, 0, int(LENGTHS.max()), seed,
                              letters=letters, **model_args(model, W))
    for a in (table, counts, starts, sample, letters, keys, left):
        a.setflags(write=False)
    return dict(table=table, counts=counts, starts=starts, sample=sample, seed=seed, W=W), letters, keys, left, gap


# ------------------------------------------------------------------------------------------- tests
def test_replica_helpers_agree_with_the_package():
    from bear_amd import kernels
    assert kernels.GEN_ID_GUMBEL == GEN_ID_GUMBEL
    for name in ALPHABETS:
        assert np.array_equal(ranks(name), kernels.score_ranks(name))
        W = len(ALPHABETS[name]) + 1
        assert BITS[W] == kernels.SCORE_BITS[W] and MAX_LAG[W] == kernels.SCORE_MAX_LAG[W]
        rng = np.random.default_rng(W)
        codes = rng.integers(0, W - 1, size=(50, 4))
        assert np.array_equal(unpack_codes(pack(codes, ranks(name), W), ranks(name), W, 4), codes)


def test_a_revisited_kmer_meets_the_same_table_values():
    """A lag-1 dna sequence of 60 letters returns to each of its four k-mers many times: per (sequence, k-mer) one row of table
    values, and different rows for different sequences and k-mers."""
    rank = ranks("dna")
    table = pack(np.arange(4)[:, None], rank, 5)
    order = np.argsort(table)
    counts = np.array([[2, 0, 1, 5, 0], [0, 3, 3, 1, 0], [4, 4, 0, 0, 0], [1, 1, 1, 1, 0]], dtype=np.int32)
    n, steps, trace = 5, 60, []
    letters = np.full((n, steps), 0xFF, dtype=np.uint8)
    replica(table[order], counts[order], rank, 1, table[np.arange(n) % 4], np.arange(n), np.full(n, steps), 0, steps, 99, van=0.3,
            letters=letters, trace=trace)
    seen = {}
    visits = 0
    for _, live, q, tv in trace:
        for i, key, row in zip(live, q, tv):
            first = seen.setdefault((int(i), int(key)), row)
            visits += first is not row
            assert np.array_equal(first, row)
    assert visits > n * (steps - 4) - 1 and len(seen) > n * 2
    rows = np.array(list(seen.values()))
    assert len({r.tobytes() for r in rows}) == len(rows)


def test_first_letter_follows_the_posterior_mean():
    """4096 replicates from one k-mer of a lag-2 table, van = 0.5: a letter drawn from a posterior sample of the row has the
    closed-form marginal (c_b + van) / sum_b (c_b + van) over the letters b < W - 1."""
    rank = ranks("dna")
    n, van = 4096, 0.5
    start = pack(np.array([[1, 3]]), rank, 5)
    table = np.sort(np.concatenate([start, pack(np.array([[0, 0], [2, 1], [3, 3]]), rank, 5)]))
    counts = np.zeros((4, 5), dtype=np.int32)
    row = np.array([7, 1, 0, 3, 9])                              # the stop's 9 takes no part
    counts[int(np.searchsorted(table, start[0]))] = row
    letters = np.full((n, 1), 0xFF, dtype=np.uint8)
    replica(table, counts, rank, 2, np.repeat(start, n), np.arange(n), np.ones(n), 0, 1, 5, van=van, letters=letters)
    p = (row[:4] + van) / (row[:4] + van).sum()
    freq = np.bincount(letters[:, 0], minlength=4)
    z = (freq - n * p) / np.sqrt(n * p * (1 - p))
    print("first-letter frequencies", freq / n, "closed form", p, "z", z)
    assert np.all(np.abs(z) < Z_MAX)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_cases_are_decided_by_a_margin(case):
    """Every step of every sequence of the cases the GPU test runs is decided by more than MIN_GAP, so the kernel's letters must
    EQUAL the replica's; and the cases do visit what they are there for."""
    inputs, letters, keys, left, gap = expected(case)
    print(case, "smallest gap", gap)
    assert gap > MIN_GAP
    assert np.all(left == 0)
    for i, n in enumerate(LENGTHS):
        assert np.all(letters[i, :n] < inputs["W"] - 1) and np.all(letters[i, n:] == 0xFF)
    assert LENGTHS.min() == 0 and LENGTHS.max() == 40 and len(set(LENGTHS.tolist())) > 30


def test_trained_cases_find_rows_and_miss_rows():
    for case in CASES:
        alphabet_name, lag, model, kind = case
        if kind != "trained" or model != "bmm":
            continue
        inputs = expected(case)[0]
        trace = []
        replica(inputs["table"], inputs["counts"], ranks(alphabet_name), lag, inputs["starts"], inputs["sample"], LENGTHS, 0, 40,
                inputs["seed"], van=0.5, letters=np.full((N_SEQ, 40), 0xFF, dtype=np.uint8), trace=trace)
        found = np.concatenate([np.isin(q, inputs["table"]) for _, _, q, _ in trace])
        assert found.any() and (lag == 1 or not found.all()), case


def test_entry_declared_bound_and_refusing():
    """Fails on the parent commit: the header declares bear_generate_steps_f64, the binding holds it, the ABI version stays 12,
    and every refusal of the header comes before any device call (this test runs without a device)."""
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    assert version == 12 == _lib.ABI_VERSION
    vp, i, u64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_double
    want = [vp, vp, u64, i, i, vp, i, i, d, d, vp, u64, vp, vp, vp, u64, u64, u64, vp, u64, vp, vp]
    assert "bear_generate_steps_f64" in _lib.SYMBOLS and sigs["bear_generate_steps_f64"] == (i, want)
    fn = _lib.lib().bear_generate_steps_f64
    assert fn.restype is i and list(fn.argtypes) == want
    assert callable(kernels.generate_steps)
    header = open(_lib.HEADER_PATH).read()
    for name, value in (("BEAR_GEN_BMM", kernels.GEN_BMM), ("BEAR_GEN_BEAR", kernels.GEN_BEAR), ("BEAR_GEN_AR", kernels.GEN_AR)):
        assert "#define %s %d" % (name, value) in header
    dna, prot = kernels.score_ranks("dna").ctypes.data, kernels.score_ranks("prot").ctypes.data
    fake = ctypes.c_void_p(8)       # a prior that is "given": never dereferenced, n_seq = 0 and every refusal comes first

    def call(lag=3, width=5, rank=dna, mode=0, get_map=0, h=1.0, van=1.0, prior=None, step0=0, n_steps=4, stride=4):
        return fn(None, None, 0, lag, width, rank, mode, get_map, h, van, prior, 1, None, None, None, 0, step0, n_steps, None, stride,
                  None, None)
    assert call() == 0 and call(lag=21) == 0 and call(lag=12, width=21, rank=prot) == 0
    assert call(mode=1, prior=fake, n_steps=1) == 0 and call(mode=2, get_map=1, prior=fake, n_steps=1) == 0
    assert call(width=4) == -1 and call(width=20, rank=prot) == -1
    assert call(lag=0) == -1 and call(lag=22) == -1 and call(lag=13, width=21, rank=prot) == -1
    assert call(mode=1, prior=fake, n_steps=2) == -1              # more than one step with a prior
    assert call(mode=1, prior=None, n_steps=1) == -1 and call(mode=2, get_map=1, prior=None, n_steps=1) == -1
    assert call(mode=2, get_map=0, prior=fake, n_steps=1) == -1 and call(mode=3) == -1
    assert call(mode=1, prior=fake, n_steps=1, h=0.0) == -1 and call(mode=1, prior=fake, n_steps=1, h=float("nan")) == -1
    assert call(van=0.0) == -1 and call(van=-1.0) == -1 and call(van=float("nan")) == -1
    assert call(step0=3, n_steps=2, stride=4) == -1 and call(step0=3, n_steps=1, stride=4) == 0
