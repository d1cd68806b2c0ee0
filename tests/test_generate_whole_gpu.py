"""GPU tests of whole-sequence generation on the device (bear_generate_whole_f64, generate_whole_kernel of kernels_generate.h;
assemble.generate_sequences).  Letters, lengths, stop flags, keys and codes are held to the NumPy replica of
tests/test_generate_whole_cpu.py and must EQUAL it: that file shows that every draw of these cases is decided by a margin no
rounding difference between host and device reaches."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_generate_cpu as g
import test_generate_whole_cpu as w
from conftest import ROOT

pytestmark = pytest.mark.gpu

L = w.MAX_LEN
FIELDS = ("letters", "keys", "left", "length", "stopped", "codes")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _i64(a, dev):
    import torch
    return torch.from_numpy(np.array(a).view(np.int64)).to(dev)


def run_case(case, dev, cuts=(L,), stepwise=False, n_seq=w.N_SEQ, sample=None):
    """A case of test_generate_whole_cpu.ALL_CASES through kernels.generate_whole, ``sum(cuts)`` steps cut into launches of ``cuts``
    steps -> a dict of FIELDS as NumPy arrays.  A model with prior rows takes one step per launch, its rows formed on the host from
    the keys; a linear case runs with ``mat`` inside the kernel, or ``stepwise`` on the rows of kernels.linear_forward_wide."""
    import torch
    from bear_amd import kernels
    name, lag, model = case
    inputs, kw = w.case_inputs(case)
    kw = dict(kw)
    W, rank, n_steps = inputs["W"], inputs["rank"], sum(cuts)
    table, counts = _i64(inputs["table"], dev), torch.from_numpy(inputs["counts"].copy()).to(dev)
    starts = w.start_keys(n_seq, rank, lag)
    keys, sample = _i64(starts, dev), _i64(inputs["sample"] if sample is None else sample, dev)
    left = torch.full((n_seq,), n_steps, dtype=torch.int32, device=dev)
    length = torch.zeros(n_seq, dtype=torch.int32, device=dev)
    stopped = torch.zeros(n_seq, dtype=torch.uint8, device=dev)
    letters = torch.full((n_seq, n_steps), 0xFF, dtype=torch.uint8, device=dev)
    codes = torch.from_numpy(g.unpack_codes(starts, rank, W, lag)).to(dev) if stepwise else torch.full((n_seq, lag), -9, dtype=torch.int8, device=dev)
    state = (table, counts, rank, lag, keys, sample, left, length, stopped, letters)
    prior = kw.pop("prior", None)
    if prior is not None and inputs["mat"] is not None and not stepwise:
        prior, kw["mat"] = None, torch.from_numpy(inputs["mat"].copy()).to(dev)
    if prior is None:
        step0 = 0
        for n in cuts:
            kernels.generate_whole(*state, step0, n, inputs["seed"], codes=codes, **kw)
            step0 += n
    else:
        mat = torch.from_numpy(inputs["mat"].copy()).to(dev) if stepwise else None
        for t in range(n_steps):
            if stepwise:
                rows = kernels.linear_forward_wide(codes, mat, lag)
            else:
                rows = torch.from_numpy(prior(keys.cpu().numpy().view(np.uint64))).to(dev)
            kernels.generate_whole(*state, t, 1, inputs["seed"], prior=rows, codes=codes, **kw)
    out = dict(letters=letters, keys=keys, left=left, length=length, stopped=stopped, codes=codes)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["keys"] = out["keys"].view(np.uint64)
    return out


def assert_equals_replica(got, want, case, n=None):
    inputs = w.case_inputs(case)[0]
    differ = np.flatnonzero((got["letters"][:n] != want["letters"]).any(axis=1))
    assert differ.size == 0, (case, "sequences that differ", differ.tolist(), "smallest gap of the case", want["gap"])
    for name in ("keys", "left", "length", "stopped"):
        assert np.array_equal(got[name][:n], want[name]), (case, name)
    assert np.array_equal(got["codes"][:n], g.unpack_codes(want["keys"], inputs["rank"], inputs["W"], inputs["lag"])), case


def assert_same_bytes(a, b, what):
    for name in FIELDS:
        assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (what, name)


@pytest.mark.parametrize("case", w.CASES, ids=w.CASE_IDS[:len(w.CASES)])
def test_bytes_equal_the_replica(case, dev):
    assert_equals_replica(run_case(case, dev), w.expected(case), case)


@pytest.mark.parametrize("case", w.LINEAR_CASES, ids=w.CASE_IDS[len(w.CASES):])
def test_linear_function_in_the_kernel_equals_its_rows_and_the_replica(case, dev):
    """``mat`` in one launch and stepwise on kernels.linear_forward_wide rows: identical bytes, and both the replica's."""
    one, steps = run_case(case, dev), run_case(case, dev, stepwise=True)
    assert_same_bytes(one, steps, case)
    assert_equals_replica(one, w.expected(case), case)
    assert_equals_replica(steps, w.expected(case), case)


@pytest.mark.parametrize("case", [("dna", 5, "bmm"), ("prot", 12, "bmm"), ("prot", 5, "bmm_map"), ("prot", 5, "lin_bear")],
                         ids=lambda c: "-".join(map(str, c)))
def test_any_cut_of_the_steps_gives_the_same_bytes(case, dev):
    whole = run_case(case, dev)
    for cuts in ((13, 35), (1,) * 48, (48, 0), (0, 7, 41)):
        assert_same_bytes(whole, run_case(case, dev, cuts), cuts)
    assert_equals_replica(whole, w.expected(case), case)


@pytest.mark.parametrize("case,n_seq", [(("prot", 5, "bmm"), w.N_SEQ), (("dna", 21, "bmm"), w.N_SEQ), (("dna", 1, "bmm"), 65),
                                        (("prot", 12, "bmm"), 65)],
                         ids=["prot-5-bmm", "dna-21-bmm", "dna-1-bmm-65", "prot-12-bmm-65"])
def test_letters_are_those_of_generate_steps(case, n_seq, dev):
    """The prefix property on the device: kernels.generate_steps from the same keys with ``left = length`` writes the same letters.
    The shortest and the longest key run 65 sequences: one more than a block of generate_steps_kernel holds at 4 lanes a sequence,
    a partly filled last group at 32."""
    import torch
    from bear_amd import kernels
    inputs, kw = w.case_inputs(case)
    sample = np.arange(n_seq, dtype=np.uint64) * np.uint64(3) + np.uint64(7)
    assert np.array_equal(sample[:w.N_SEQ], inputs["sample"])
    got = run_case(case, dev, n_seq=n_seq, sample=sample)
    if n_seq != w.N_SEQ:
        want = w.run_replica(case, n_seq=n_seq, sample=sample)
        assert want["gap"] > g.MIN_GAP
        assert_equals_replica(got, want, case)
    keys, sample = _i64(w.start_keys(n_seq, inputs["rank"], inputs["lag"]), dev), _i64(sample, dev)
    left = torch.from_numpy(got["length"].copy()).to(dev)
    letters = torch.full((n_seq, L), 0xFF, dtype=torch.uint8, device=dev)
    kernels.generate_steps(_i64(inputs["table"], dev), torch.from_numpy(inputs["counts"].copy()).to(dev), inputs["rank"], inputs["lag"],
                           keys, sample, left, letters, 0, L, inputs["seed"], **kw)
    assert np.array_equal(letters.cpu().numpy(), got["letters"]) and got["length"].max() > 0
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), got["keys"]) and not bool(left.any())


@pytest.mark.parametrize("case,n_seq", [(("dna", 5, "bmm"), 70001), (("prot", 5, "bmm"), 70001), (("prot", 5, "lin_bear"), 4097)],
                         ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_a_sequence_is_the_same_wherever_it_sits(case, n_seq, dev):
    """Sequence i carries the sample index of sequence i % 37 and must equal it: in a partial last block, and -- with ``mat``, whose
    grid is capped at 512 blocks of 8 sequences -- on the second trip of the grid-stride loop; the first 37 are the replica's."""
    steps = 4
    sample = w.case_inputs(case)[0]["sample"][np.arange(n_seq) % w.N_SEQ]
    got = run_case(case, dev, cuts=(steps,), n_seq=n_seq, sample=sample)
    for name in FIELDS:
        assert np.array_equal(got[name], got[name][:w.N_SEQ][np.arange(n_seq) % w.N_SEQ]), name
    want = w.run_replica(case, n_steps=steps)
    assert want["gap"] > g.MIN_GAP
    assert_equals_replica(got, want, case, n=w.N_SEQ)


DET_CASES = [("dna", 21, "bmm"), ("prot", 5, "bear"), ("prot", 12, "bmm_map"), ("prot", 5, "lin_bear")]

_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/oracle"]
import numpy as np
import torch
from bear_amd import _lib
import test_generate_whole_gpu as t
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
np.save(sys.argv[2], np.frombuffer(t.det_bytes(torch.device("cuda", 0)), dtype=np.uint8))
"""


def det_bytes(dev):
    return b"".join(run_case(case, dev)[name].tobytes() for case in DET_CASES for name in FIELDS)


def test_deterministic_library_gives_the_same_bytes(dev, tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    here = det_bytes(dev)
    script = tmp_path / "det_generate_whole.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npy")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert np.load(tmp_path / "det.npy").tobytes() == here


# ------------------------------------------------------------------------------------------- assemble.generate_sequences
MIXED = ["MKVLAARND", "ACDEFGHIKL", "MKTAYIAKQR", "GSHMKV", "LLAARNDCEQ", "MKVLA", "ACDKLMN", "WYVMKVLAAR", "NDCEQGHILK", "MFPSTWYV",
         "ARNDARND", "KLMKLMKL"]


def _count_launches(monkeypatch):
    from bear_amd import kernels
    calls = []
    launch = kernels._launch
    monkeypatch.setattr(kernels, "_launch", lambda device, name, *a: (calls.append(name), launch(device, name, *a))[1])
    return calls


def _replica_of(counter, prompts, num_to_gen, max_len, seed, **model):
    """generate_sequences' answer from the replica over the counter's own table: start keys of the padded prompts, sample index
    prompt * num_to_gen + replicate."""
    name, lag, W = counter.alphabet_name, counter.lag, counter.width
    rank = g.ranks(name)
    code = {ch: c for c, ch in enumerate(g.ALPHABETS[name])}
    code["["] = W
    starts = g.pack(np.array([[code[ch] for ch in ("[" * lag + p)[-lag:]] for p in prompts]), rank, W)
    table, counts = counter.keys.cpu().numpy().view(np.uint64), counter.counts_by_key.cpu().numpy()
    n = len(prompts) * num_to_gen
    strings, stopped, gap = w.replica_strings(table, counts, name, lag, np.repeat(starts, num_to_gen), np.arange(n), max_len, seed, **model)
    assert gap > g.MIN_GAP, gap
    strings = [prompts[i // num_to_gen] + s for i, s in enumerate(strings)]
    return np.array(strings, dtype=str).reshape(len(prompts), num_to_gen), stopped.reshape(len(prompts), num_to_gen), starts


def test_generate_sequences_bmm(dev, tmp_path, monkeypatch):
    from bear_amd import assemble, get_var_probs, kernels
    P = w.PERIODIC
    counter = get_var_probs.DeviceCounter.from_sequences(P["strings"], P["lag"], reverse=False, alphabet_name=P["name"])
    calls = _count_launches(monkeypatch)
    seqs, stopped = assemble.generate_sequences(counter, P["n"], P["max_len"], van=P["van"], seed=P["seed"], save_folder=str(tmp_path / "out"))
    assert calls.count("bear_generate_whole_f64") == 1 and "bear_generate_steps_f64" not in calls      # one launch for everything
    assert seqs.shape == (1, P["n"]) and stopped.shape == (1, P["n"]) and stopped.dtype == bool
    assert seqs.tolist() == [["ACDEFGHIKL"] * P["n"]] and stopped.all()
    assert (tmp_path / "out" / "seqs.fa").read_text() == "".join(">seq0_rep%d\nACDEFGHIKL\n" % j for j in range(P["n"]))
    # a table with something to choose: same seed, same strings; another seed differs; the strings are the replica's
    counter = get_var_probs.DeviceCounter.from_sequences(MIXED, 3, reverse=False, alphabet_name="prot")
    num, max_len = 40, 12
    a, sa = assemble.generate_sequences(counter, num, max_len, van=0.5, seed=11)
    b, sb = assemble.generate_sequences(counter, num, max_len, van=0.5, seed=11)
    c, _ = assemble.generate_sequences(counter, num, max_len, van=0.5, seed=12)
    assert np.array_equal(a, b) and np.array_equal(sa, sb) and not np.array_equal(a, c) and len(set(a[0].tolist())) > num // 2
    want, want_stopped, _ = _replica_of(counter, [""], num, max_len, 11, van=0.5)
    assert np.array_equal(a, want) and np.array_equal(sa, want_stopped)
    assert sa.any() and not sa.all()
    assert all(len(s) == max_len for s in a[~sa]) and all(len(s) <= max_len for s in a[sa]) and set("".join(a[0])) <= set(g.ALPHABETS["prot"])
    # get_map: the table at its MAP value
    m, sm = assemble.generate_sequences(counter, num, max_len, van=0.5, seed=11, get_map=True)
    want, want_stopped, _ = _replica_of(counter, [""], num, max_len, 11, van=0.5, get_map=True)
    assert np.array_equal(m, want) and np.array_equal(sm, want_stopped)
    # prompts: shorter than the lag, longer, empty -- prefixes of their continuations, from the keys of the padded prompts
    prompts = ["MK", "ACDEFGH", ""]
    seen = []
    whole = kernels.generate_whole
    monkeypatch.setattr(kernels, "generate_whole", lambda *a, **kw: (seen.append(a[4].clone()), whole(*a, **kw))[1])
    p, sp = assemble.generate_sequences(counter, 5, max_len, van=0.5, seed=4, prompts=prompts)
    want, want_stopped, starts = _replica_of(counter, prompts, 5, max_len, 4, van=0.5)
    assert len(seen) == 1 and np.array_equal(seen[0].cpu().numpy().view(np.uint64), np.repeat(starts, 5))
    assert p.shape == (3, 5) and all(s.startswith(prompts[i]) for i in range(3) for s in p[i])
    assert np.array_equal(p, want) and np.array_equal(sp, want_stopped)
    for i in range(3):
        assert all(len(s) - len(prompts[i]) == max_len for s in p[i][~sp[i]])
    # nothing to generate
    e, se = assemble.generate_sequences(counter, 3, 0, van=0.5, seed=4, prompts=["MK"])
    assert e.tolist() == [["MK"] * 3] and not se.any()


def test_generate_sequences_trained_linear_model(dev, monkeypatch):
    """make_ar_func_linear(3, 20): one launch by default (the function inside the kernel), a launch and an AR call per step with
    ``stepwise``, the same strings both ways; the per-step path looks at most every 16 steps whether anything is left."""
    import torch
    from bear_amd import ar_funcs, assemble, get_var_probs
    counter = get_var_probs.DeviceCounter.from_sequences(MIXED, 3, reverse=False, alphabet_name="prot")
    ar_func, _ = ar_funcs.make_ar_func_linear(3, 20, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    assert ar_func.fused and ar_func.linear_mat.is_cuda
    calls = _count_launches(monkeypatch)
    looks = []
    any_left = assemble._any_left
    monkeypatch.setattr(assemble, "_any_left", lambda left: (looks.append(1), any_left(left))[1])
    num, max_len = 30, 40
    for kw in (dict(h=0.5), dict(get_map=True)):
        del calls[:], looks[:]
        one, s_one = assemble.generate_sequences(counter, num, max_len, ar_func=ar_func, seed=8, prompts=["", "MKV"], **kw)
        assert calls.count("bear_generate_whole_f64") == 1 and "bear_linear_forward_wide_f64" not in calls and not looks
        del calls[:]
        steps, s_steps = assemble.generate_sequences(counter, num, max_len, ar_func=ar_func, seed=8, prompts=["", "MKV"], stepwise=True, **kw)
        n = calls.count("bear_generate_whole_f64")
        assert 1 < n <= max_len and calls.count("bear_linear_forward_wide_f64") == n
        assert len(looks) <= math.ceil(max_len / 16) and len(looks) == (n - (n == max_len)) // 16
        assert np.array_equal(one, steps) and np.array_equal(s_one, s_steps)
        assert one.shape == (2, num) and s_one.any() and len(set(one[0].tolist())) > 1 and all(s.startswith("MKV") for s in one[1])


def test_refusals_come_before_any_launch(dev, monkeypatch):
    from bear_amd import assemble, get_var_probs, kernels
    counter = get_var_probs.DeviceCounter.from_sequences(MIXED, 3, reverse=False, alphabet_name="prot")
    no_end = get_var_probs.DeviceCounter.from_sequences(MIXED, 3, reverse=False, no_end=True, alphabet_name="prot")

    def no_launch(*a):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(kernels, "_launch", no_launch)
    with pytest.raises(ValueError, match="no_end"):
        assemble.generate_sequences(no_end, 2, 5, van=0.5, seed=1)
    with pytest.raises(ValueError, match="'B'"):
        assemble.generate_sequences(counter, 2, 5, van=0.5, seed=1, prompts=["MK", "MBK"])
    with pytest.raises(ValueError, match=r"'\['"):
        assemble.generate_sequences(counter, 2, 5, van=0.5, seed=1, prompts=["[MK"])
    with pytest.raises(ValueError, match="max_len"):
        assemble.generate_sequences(counter, 2, -1, van=0.5, seed=1)
    with pytest.raises(ValueError, match="one model"):
        assemble.generate_sequences(counter, 2, 5, seed=1)
    with pytest.raises(ValueError, match="one model"):
        assemble.generate_sequences(counter, 2, 5, van=0.5, ar_func=lambda codes: None, h=1.0, seed=1)
    with pytest.raises(ValueError, match="h"):
        assemble.generate_sequences(counter, 2, 5, ar_func=lambda codes: None, seed=1)
    with pytest.raises(TypeError):
        assemble.generate_sequences(lambda kmers: np.zeros((len(kmers), 21)), 2, 5, van=0.5, seed=1)      # a host counter
    # the wrapper: what generate_steps refuses, and what is new
    import torch
    n, lag = 6, 3
    rank = kernels.score_ranks("prot")
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    sample = torch.arange(n, dtype=torch.int64, device=dev)
    left = torch.full((n,), 4, dtype=torch.int32, device=dev)
    length = torch.zeros(n, dtype=torch.int32, device=dev)
    stopped = torch.zeros(n, dtype=torch.uint8, device=dev)
    letters = torch.full((n, 4), 0xFF, dtype=torch.uint8, device=dev)
    prior = torch.full((n, 21), 1 / 21, dtype=torch.float64, device=dev)
    mat = torch.zeros((lag, 21, 21), dtype=torch.float64, device=dev)
    for bad in (dict(n_steps=5, van=1.0), dict(n_steps=2, prior=prior, h=1.0), dict(n_steps=1, prior=prior), dict(n_steps=1),
                dict(n_steps=1, van=0.0), dict(n_steps=1, prior=prior, mat=mat, h=1.0), dict(n_steps=4, mat=mat), dict(n_steps=4, mat=mat[:2], h=1.0),
                dict(n_steps=4, mat=mat.float(), h=1.0), dict(n_steps=1, van=1.0, length=length.long()), dict(n_steps=1, van=1.0, stopped=stopped[:5]),
                dict(n_steps=1, van=1.0, stopped=None)):
        kw = dict(bad)
        a = [counter.keys, counter.counts_by_key, rank, lag, keys, sample, left, kw.pop("length", length), kw.pop("stopped", stopped), letters]
        with pytest.raises(ValueError):
            kernels.generate_whole(*a, 0, kw.pop("n_steps"), 1, **kw)
    drank = kernels.score_ranks("dna")                        # mat at width 5
    with pytest.raises(ValueError, match="21"):
        kernels.generate_whole(torch.zeros(0, dtype=torch.int64, device=dev), None, drank, lag, keys, sample, left, length, stopped, letters,
                               0, 4, 1, mat=mat, h=1.0)
