"""CPU tests of whole-sequence generation on the device (generate_whole_kernel of kernels_generate.h, bear_generate_whole_f64,
assemble.generate_sequences): a NumPy replica of the kernel's rule -- ``test_generate_cpu.replica`` with the stop drawn like a
letter -- on the oracle's counter streams, the margin that lets the GPU comparison be exact, what the rule promises (the first draw
follows the posterior mean, the stop included; the letters are those of the flank kernel's rule), and the entry in the header and
the binding.  ``tests/test_generate_whole_gpu.py`` compares the kernel's bytes with the replica's."""
import ctypes
import functools

import numpy as np
import pytest

import bear_oracle as o
import test_generate_cpu as g
from util import abi_header

MAX_LEN = 48
N_SEQ = 37                           # not a multiple of the 32 (W = 5) or 8 (W = 21) sequences of a block


def replica_whole(table, counts, rank, lag, keys, sample, left, length, stopped, step0, n_steps, seed, van=None, prior=None, h=None,
                  get_map=False, letters=None):
    """The rule of generate_whole_kernel: ``test_generate_cpu.replica`` over all W columns.  Where the stop (column W - 1) wins,
    ``stopped`` is set, ``left`` becomes 0, nothing is written and the key stays; a letter is written, shifts the key and adds 1 to
    ``length``.  ``prior``: None or a function keys -> [n, W].  The inputs are left alone (``letters`` is filled in place).  Returns
    ``(keys, left, length, stopped, smallest best-minus-second-best score)``."""
    W = rank.size - 1
    bits, mask = np.uint64(g.BITS[W]), np.uint64((1 << (g.BITS[W] * lag)) - 1)
    keys, left = np.array(keys, dtype=np.uint64), np.array(left, dtype=np.int64)
    length, stopped = np.array(length, dtype=np.int64), np.array(stopped, dtype=np.uint8)
    sample = np.asarray(sample, dtype=np.uint64)
    b = np.arange(W, dtype=np.uint64)[None, :]
    gap = np.inf
    for k in range(n_steps):
        live = np.flatnonzero(left > 0)
        if live.size == 0:
            break
        t, q, s = step0 + k, keys[live], sample[live][:, None]
        c = np.zeros((live.size, W))
        if table.size:
            pos = np.minimum(np.searchsorted(table, q), table.size - 1)
            found = table[pos] == q
            c[found] = counts[pos[found]]
        if prior is None:
            conc = van + c
        elif h is None:
            conc = prior(q)
        else:
            conc = prior(q) * (1.0 / h) + c
        with np.errstate(over="ignore"):
            if get_map:
                tv = np.log(conc)
            else:
                tkey = o._cell_key(seed, 0, s, o._mix64(q)[:, None] + b)
                tv = o.log_gamma_keys(conc.reshape(-1), tkey.reshape(-1)).reshape(conc.shape)
            gumbel = -np.log(-np.log(o._u01(o._cell_key(seed, g.GEN_ID_GUMBEL, s, np.uint64(t * W) + b))))
        score = tv + gumbel
        best = np.argmax(score, axis=1)                        # the lowest letter with the largest score
        top = np.sort(score, axis=1)
        gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
        stop = best == W - 1
        on, letter = live[~stop], best[~stop]
        with np.errstate(over="ignore"):
            keys[on] = ((q[~stop] << bits) | rank[letter].astype(np.uint64)) & mask
        letters[on, t] = letter
        length[on] += 1
        left[on] -= 1
        stopped[live[stop]] = 1
        left[live[stop]] = 0
    return keys, left, length, stopped, gap


def count_symbols(strings, rank, lag, times=1):
    """``(table uint64 [N] ascending, counts int32 [N, W])`` of strings of letter codes 0 .. W - 2, counted WITH their ends: the
    symbols of a string are ``lag`` starts (code W), its letters and one stop (column W - 1); every window of ``lag + 1`` symbols is
    a transition, counted ``times`` times."""
    W = rank.size - 1
    windows = np.concatenate([np.lib.stride_tricks.sliding_window_view(np.concatenate([np.full(lag, W), s, [W - 1]]).astype(np.int64),
                                                                       lag + 1) for s in strings])
    table, inverse = np.unique(g.pack(windows[:, :lag], rank, W), return_inverse=True)
    counts = np.zeros((table.size, W), dtype=np.int32)
    np.add.at(counts, (inverse.reshape(-1), windows[:, lag]), times)
    return table, counts


def start_keys(n, rank, lag):
    W = rank.size - 1
    return np.repeat(g.pack(np.full((1, lag), W), rank, W), n)


def linear_rows(keys, mat, rank, lag):
    """The linear AR function on the codes of the end keys: the max-shifted softmax of sum_l mat[l, code_l, :] ('[' = 20)."""
    codes = g.unpack_codes(keys, rank, 21, lag).astype(np.int64)
    z = mat[np.arange(lag)[None, :], codes].sum(axis=1)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------- the cases both test files run
CASES = [(name, lag, model) for name in ("dna", "prot") for lag in (1, 5, g.MAX_LAG[len(g.ALPHABETS[name]) + 1]) for model in g.MODELS]
LINEAR_CASES = [("prot", lag, model) for lag in (1, 5, 12) for model in ("lin_bear", "lin_ar_map")]
ALL_CASES = CASES + LINEAR_CASES
CASE_IDS = ["-".join(map(str, c)) for c in ALL_CASES]


def case_seed(case):
    name, lag, model = case
    if model.startswith("lin_"):
        return 5000 + 10 * lag + ("lin_bear", "lin_ar_map").index(model)
    return 2000 + 100 * (len(g.ALPHABETS[name]) + 1) + 10 * lag + g.MODELS.index(model)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """``(inputs, model arguments of the replica)`` of a case; a linear case carries ``mat`` [lag, 21, 21] among the inputs."""
    name, lag, model = case
    W, rank, seed = len(g.ALPHABETS[name]) + 1, g.ranks(name), case_seed(case)
    rng = np.random.default_rng(seed)
    if model.startswith("lin_"):
        mat = rng.normal(size=(lag, 21, 21)) * 0.5
        kw = dict(prior=functools.partial(linear_rows, mat=mat, rank=rank, lag=lag), **(dict(h=0.25) if model == "lin_bear" else dict(get_map=True)))
    else:
        mat, kw = None, g.model_args(model, W)
    strings = []
    for _ in range(8):
        n = int(rng.integers(6, 31))
        strings.append(rng.integers(0, W - 1, size=n))
    table, counts = count_symbols(strings, rank, lag, times=3)
    sample = np.arange(N_SEQ, dtype=np.uint64) * np.uint64(3) + np.uint64(7)
    inputs = dict(table=table, counts=counts, starts=start_keys(N_SEQ, rank, lag), sample=sample, seed=seed, W=W, rank=rank, lag=lag, mat=mat)
    for a in inputs.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inputs, kw


def run_replica(case, n_steps=MAX_LEN, n_seq=N_SEQ, sample=None):
    inputs, kw = case_inputs(case)
    sample = inputs["sample"] if sample is None else sample
    letters = np.full((n_seq, n_steps), 0xFF, dtype=np.uint8)
    keys, left, length, stopped, gap = replica_whole(inputs["table"], inputs["counts"], inputs["rank"], inputs["lag"],
                                                     start_keys(n_seq, inputs["rank"], inputs["lag"]), sample, np.full(n_seq, n_steps),
                                                     np.zeros(n_seq), np.zeros(n_seq), 0, n_steps, inputs["seed"], letters=letters, **kw)
    return dict(letters=letters, keys=keys, left=left, length=length, stopped=stopped, gap=gap)


@functools.lru_cache(maxsize=None)
def expected(case):
    """The replica's answer for a case, computed once and left unchanged."""
    out = run_replica(case)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# the periodic end-to-end case of the GPU file: whichever seed makes the replica spell the period ten times is the seed there
PERIODIC = dict(strings=["ACDEFGHIKL"] * 400, name="prot", lag=3, van=0.01, n=10, seed=3, max_len=30)


def string_table(strings, name, lag):
    code = {ch: c for c, ch in enumerate(g.ALPHABETS[name])}
    return count_symbols([np.array([code[ch] for ch in s], dtype=np.int64) for s in strings], g.ranks(name), lag)


def replica_strings(table, counts, name, lag, starts, sample, max_len, seed, **model):
    """``(strings, stopped, smallest gap)``: generate_sequences' answer from the replica, without the prompts."""
    n = len(starts)
    letters = np.full((n, max_len), 0xFF, dtype=np.uint8)
    _, _, length, stopped, gap = replica_whole(table, counts, g.ranks(name), lag, starts, sample, np.full(n, max_len), np.zeros(n),
                                               np.zeros(n), 0, max_len, seed, letters=letters, **model)
    return ["".join(g.ALPHABETS[name][b] for b in row[:m]) for row, m in zip(letters, length)], stopped.astype(bool), gap


# ------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("case", ALL_CASES, ids=CASE_IDS)
def test_gpu_cases_are_decided_by_a_margin(case):
    """Every draw of every case the GPU test runs is decided by more than MIN_GAP, so the kernel's bytes must EQUAL the replica's."""
    want = expected(case)
    print(case, "smallest gap", want["gap"], "stopped", int(want["stopped"].sum()), "of", N_SEQ, "zero lengths", int((want["length"] == 0).sum()))
    assert want["gap"] > g.MIN_GAP
    W = case_inputs(case)[0]["W"]
    for i in range(N_SEQ):
        n = want["length"][i]
        assert np.all(want["letters"][i, :n] < W - 1) and np.all(want["letters"][i, n:] == 0xFF)
        assert want["left"][i] == (0 if want["stopped"][i] else MAX_LEN - n) and (want["stopped"][i] or n == MAX_LEN)


def test_cases_stop_are_cut_and_stop_at_once():
    """Across the cases some sequences stop, some are cut at MAX_LEN, and some draw the stop first (length 0)."""
    stopped = np.concatenate([expected(c)["stopped"] for c in ALL_CASES]).astype(bool)
    length = np.concatenate([expected(c)["length"] for c in ALL_CASES])
    assert stopped.any() and (~stopped).any() and np.all(length[~stopped] == MAX_LEN)
    assert np.any(stopped & (length == 0)) and np.any(stopped & (length > 0))


@pytest.mark.parametrize("case", ALL_CASES, ids=CASE_IDS)
def test_letters_are_those_of_the_flank_rule(case):
    """The prefix property: ``test_generate_cpu.replica`` (the rule of generate_steps_kernel, which never draws the stop) from the
    same keys, sample indices and seed, asked for ``length[i]`` letters, writes the letters of ``replica_whole``."""
    inputs, kw = case_inputs(case)
    want = expected(case)
    letters = np.full((N_SEQ, MAX_LEN), 0xFF, dtype=np.uint8)
    keys, left, _ = g.replica(inputs["table"], inputs["counts"], inputs["rank"], inputs["lag"], inputs["starts"], inputs["sample"],
                              want["length"], 0, MAX_LEN, inputs["seed"], letters=letters, **kw)
    assert np.array_equal(letters, want["letters"]) and np.array_equal(keys, want["keys"]) and not left.any()


def test_first_draw_follows_the_posterior_mean_stop_included():
    """4096 replicates from the start row of a lag-2 dna table with letter counts 7, 1, 0, 3 and stop count 9, van = 0.5: the first
    draw is the stop with probability (9 + van) / sum(c + van), and each letter with its own share."""
    rank = g.ranks("dna")
    n, van, lag = 4096, 0.5, 2
    start = start_keys(1, rank, lag)
    table = np.sort(np.concatenate([start, g.pack(np.array([[0, 0], [2, 1], [3, 3]]), rank, 5)]))
    counts = np.zeros((4, 5), dtype=np.int32)
    row = np.array([7, 1, 0, 3, 9])
    counts[int(np.searchsorted(table, start[0]))] = row
    letters = np.full((n, 1), 0xFF, dtype=np.uint8)
    _, left, length, stopped, _ = replica_whole(table, counts, rank, lag, np.repeat(start, n), np.arange(n), np.ones(n), np.zeros(n),
                                                np.zeros(n), 0, 1, 5, van=van, letters=letters)
    assert not left.any() and np.array_equal(stopped == 1, length == 0) and np.array_equal(letters[:, 0] == 0xFF, stopped == 1)
    p = (row + van) / (row + van).sum()
    freq = np.bincount(np.where(stopped == 1, 4, letters[:, 0]), minlength=5)
    z = (freq - n * p) / np.sqrt(n * p * (1 - p))
    print("first-draw frequencies", freq / n, "closed form", p, "z", z)
    assert np.all(np.abs(z) < g.Z_MAX)


def test_periodic_case_spells_its_period_and_stops():
    P = PERIODIC
    table, counts = string_table(P["strings"], P["name"], P["lag"])
    strings, stopped, gap = replica_strings(table, counts, P["name"], P["lag"], start_keys(P["n"], g.ranks(P["name"]), P["lag"]),
                                            np.arange(P["n"]), P["max_len"], P["seed"], van=P["van"])
    print("smallest gap", gap)
    assert strings == ["ACDEFGHIKL"] * P["n"] and stopped.all() and gap > g.MIN_GAP


def test_entry_declared_bound_and_refusing():
    """The header declares bear_generate_whole_f64, the binding holds it, the ABI version stays 12, and every refusal of the header
    comes before any device call (this test runs without a device)."""
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    assert version == 12 == _lib.ABI_VERSION
    vp, i, u64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_double
    want = [vp, vp, u64, i, i, vp, i, i, d, d, vp, vp, u64, vp, vp, vp, vp, vp, u64, u64, u64, vp, u64, vp, vp]
    assert "bear_generate_whole_f64" in _lib.SYMBOLS and sigs["bear_generate_whole_f64"] == (i, want)
    fn = _lib.lib().bear_generate_whole_f64
    assert fn.restype is i and list(fn.argtypes) == want
    assert callable(kernels.generate_whole)
    dna, prot = kernels.score_ranks("dna").ctypes.data, kernels.score_ranks("prot").ctypes.data
    fake = ctypes.c_void_p(8)       # a pointer that is "given": never dereferenced, every refusal comes first

    def call(lag=3, width=5, rank=dna, mode=0, get_map=0, h=1.0, van=1.0, prior=None, mat=None, step0=0, n_steps=4, stride=4, n_seq=0,
             state=(None, None, None, None, None), letters=None):
        return fn(None, None, 0, lag, width, rank, mode, get_map, h, van, prior, mat, 1, *state, n_seq, step0, n_steps, letters, stride,
                  None, None)
    wide = dict(width=21, rank=prot)
    assert call() == 0 and call(lag=21) == 0 and call(lag=12, **wide) == 0
    assert call(mode=1, prior=fake, n_steps=1) == 0 and call(mode=2, get_map=1, prior=fake, n_steps=1) == 0
    assert call(mode=1, mat=fake, **wide) == 0 and call(mode=2, get_map=1, mat=fake, n_steps=40, stride=40, **wide) == 0
    # everything bear_generate_steps_f64 refuses
    assert call(width=4) == -1 and call(width=20, rank=prot) == -1
    assert call(lag=0) == -1 and call(lag=22) == -1 and call(lag=13, **wide) == -1
    assert call(mode=1, prior=fake, n_steps=2) == -1              # more than one step with a prior
    assert call(mode=1, n_steps=1) == -1 and call(mode=2, get_map=1, n_steps=1) == -1 and call(mode=1, **wide) == -1      # no rows
    assert call(mode=2, get_map=0, prior=fake, n_steps=1) == -1 and call(mode=2, get_map=0, mat=fake, **wide) == -1 and call(mode=3) == -1
    assert call(mode=1, prior=fake, n_steps=1, h=0.0) == -1 and call(mode=1, mat=fake, h=float("nan"), **wide) == -1
    assert call(van=0.0) == -1 and call(van=-1.0) == -1 and call(van=float("nan")) == -1
    assert call(step0=3, n_steps=2, stride=4) == -1 and call(step0=3, n_steps=1, stride=4) == 0
    # ... and what is new here
    assert call(mode=1, prior=fake, mat=fake, n_steps=1, **wide) == -1          # both sources of rows
    assert call(mode=1, mat=fake) == -1 and call(mat=fake) == -1                # mat at width 5
    # a missing or misaligned length / stopped: refused once there are sequences, before the device is touched
    odd = ctypes.c_void_p(10)
    for state in ((fake, fake, fake, None, fake), (fake, fake, fake, fake, None), (fake, fake, fake, odd, fake), (None, fake, fake, fake, fake)):
        assert call(n_seq=1, state=state, letters=fake) == -1, state
    assert call(n_seq=1, mode=1, mat=odd, state=(fake,) * 5, letters=fake, **wide) == -1
