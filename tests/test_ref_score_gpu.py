"""GPU tests of bear_ref models downstream of training: bear_ref_prior_rows_f64 (ref_prior_rows_kernel of kernels_refscore.h) bit
for bit against the NumPy replica of tests/test_ref_score_cpu.py; get_bear_probs / get_bear_probs_seqs with ``ref_model=`` /
``ref_counter=`` against the existing device path handed the same rows; bear_generate_whole_ref_f64 (generate_whole_ref_kernel of
kernels_generate.h) and assemble.generate_sequences byte for byte against the replica; a train-then-use round trip; the
deterministic library; the refusals."""
import configparser
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_generate_cpu as g
import test_generate_whole_cpu as w
import test_ref_score_cpu as r
from conftest import ROOT

pytestmark = pytest.mark.gpu

L = r.MAX_LEN
FIELDS = ("letters", "keys", "left", "length", "stopped", "codes")
EPS = r.EPS


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _i64(a, dev):
    import torch
    return torch.from_numpy(np.array(a).view(np.int64)).to(dev)


def _counts(a, dev):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.int32)).to(dev)


# ------------------------------------------------------------------------------------------- ref_prior_rows
@pytest.fixture(scope="module")
def prior_inputs():
    """Per width: a reference table of ~300 keys with the special rows of the CPU file among its count rows, 1025 unsorted query
    keys -- present, absent, repeated -- their net rows, and the replica's answers for both net functions, computed once."""
    out = {}
    for W in (5, 21):
        rng = np.random.default_rng(40 + W)
        rows = np.concatenate([r.special_rows(W, rng), rng.integers(0, 40, size=(270, W))])
        table = np.sort(rng.choice(2 ** 40, size=rows.shape[0], replace=False).astype(np.uint64))
        counts = rows.astype(np.uint32).view(np.int32)
        query = np.concatenate([table, rng.integers(0, 2 ** 40, size=1025 - table.size).astype(np.uint64)])[rng.permutation(1025)]
        query[:3] = table[1]                                   # the huge count first, three times over
        net = rng.dirichlet(np.full(W, 0.5), size=1025)
        tau, nw = 0.2, 0.3
        want = {(n_ref, given): r.ref_rows_replica(query, table[:n_ref], counts[:n_ref], net if given else None, tau, nw)
                for n_ref in (0, 1, table.size) for given in (False, True)}
        out[W] = dict(table=table, counts=counts, query=query, net=net, tau=tau, nw=nw, want=want)
    return out


@pytest.mark.parametrize("W", [5, 21])
def test_prior_rows_equal_the_replica_bit_for_bit(W, dev, prior_inputs):
    import torch
    from bear_amd import kernels
    P = prior_inputs[W]
    assert 290 <= P["table"].size <= 310
    for n_ref in (0, 1, P["table"].size):
        table = _i64(P["table"][:n_ref], dev)
        counts = torch.from_numpy(P["counts"][:n_ref].copy()).to(dev) if n_ref else None
        for given in (False, True):
            for n_query in (0, 1, 63, 64, 65, 1025):
                net = torch.from_numpy(P["net"][:n_query].copy()).to(dev) if given else None
                got = kernels.ref_prior_rows(table, counts, _i64(P["query"][:n_query], dev), net, P["tau"], P["nw"], width=W).cpu().numpy()
                want = P["want"][n_ref, given][:n_query]
                differ = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1)) if n_query else np.zeros(0)
                assert got.shape == (n_query, W) and differ.size == 0, \
                    (W, n_ref, given, n_query, differ[:5].tolist(), got[differ[:1]].tolist(), want[differ[:1]].tolist())
    found = np.isin(P["query"], P["table"])
    assert found.any() and (~found).any() and not np.all(np.diff(P["query"].astype(np.int64)) >= 0)


def test_prior_rows_against_the_training_forward(dev, prior_inputs):
    """Width 5: kernels.ref_mix_forward on the fp64 reference rows of the same k-mers, plus eps -- bear_ref's training forward,
    which forms exp(-tau) on the device: 1e-14, not bits."""
    import torch
    from bear_amd import bear_ref, get_var_probs, kernels
    P = prior_inputs[5]
    rng = np.random.default_rng(3)
    kmers = np.array([[ord("ACGT["[c]) for c in row] for row in rng.integers(0, 5, size=(200, 4))], dtype=np.uint8)
    kmers = np.unique(kmers, axis=0)
    counts = rng.integers(0, 60, size=(kmers.shape[0], 5)).astype(np.int32)
    counts[0] = 0
    counts[1, 2] = np.uint32(4_000_000_000).astype(np.int32)
    ref_counter = get_var_probs.DeviceCounter(torch.from_numpy(kmers).to(dev), torch.from_numpy(counts).to(dev), "dna")
    keys = torch.cat([ref_counter.keys.flip(0), torch.tensor([8 ** 4 - 1, 4681], dtype=torch.int64, device=dev)])      # two the table may lack
    net = torch.from_numpy(rng.dirichlet(np.full(5, 0.5), size=keys.numel())).to(dev)
    for tau, nw in r.MODELS:
        got = kernels.ref_prior_rows(ref_counter.keys, ref_counter.counts_by_key, keys, net, tau, nw)
        want = kernels.ref_mix_forward(net, bear_ref._ref_input(ref_counter.rows_of_keys(keys)),
                                       torch.tensor(math.log(tau), dtype=torch.float64, device=dev),
                                       torch.tensor(math.log(nw), dtype=torch.float64, device=dev)) + EPS
        err = ((got - want).abs() / want.abs()).max().item()
        print(f"tau {tau:.3g} nw {nw:.3g}: largest relative difference to ref_mix_forward {err:.2e}")
        assert torch.allclose(got, want, rtol=r.RTOL, atol=0)


# ------------------------------------------------------------------------------------------- scoring
PROT_TRAIN = ["MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQAPILSRVGDGTQDNLSGAEKAVQVKVK", "MKVLAARNDCEQGHILKMFPSTWYV", "ACDEFGHIKLMNPQRSTVWY",
              "MKTAYIAKQRGSHMKVLAARND", "LLAARNDCEQMKTAYIAKQRQISF", "WYVMKVLAARNDCEQ"]
PROT_REF = ["MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQAPILSRVGDGTQDNLSG", "MKTAYLAKQRQISFVRSHFSRQ", "ACDEFGHIKLMNPQRSTVWY", "GGSGGSGGSMKV",
            "NDCEQGHILKMFPSTW"]
DNA_TRAIN = ["ACGTTGCAAGTCACGTTGCAAGTCGGATCCATGCATGCAAGTCACGT", "ACACACACACACGTGTGTGT", "TTTGGGCCCAAATTTGGGCCC", "GATTACAGATTACAGATTACA",
             "ACGTTGCAAGTCGGATCC"]
DNA_REF = ["ACGTTGCAAGTCACGTTGCATGTCGGATCCATGCATGCAAGTCACGT", "ACACACACTCACGTGTGTGT", "CCCCCCGGGGGGAAAT", "GATTACA"]
WT = {"prot": "MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQAPILSRV", "dna": "ACGTTGCAAGTCACGTTGCAAGTCGGATCCATGCATGCAA"}       # 40 residues
HS = [0.3, 4.0]
VANS = [0.1, 1.0, 10.0]


def _variants(name, rng):
    """30 substitutions of the wild type, first and last position among them."""
    letters, wt = g.ALPHABETS[name], WT[name]
    pos = [0, len(wt) - 1] + rng.integers(0, len(wt), size=28).tolist()
    return [f"{wt[p]}{p}{letters[(letters.index(wt[p]) + 1 + int(rng.integers(0, len(letters) - 1))) % len(letters)]}" for p in pos]


def _sequences(name, rng):
    """12 sequences of 5 to 60 letters: pieces of the train and reference strings and random letters."""
    letters = g.ALPHABETS[name]
    pool = (PROT_TRAIN + PROT_REF) if name == "prot" else (DNA_TRAIN + DNA_REF)
    lens = [5, 60] + rng.integers(5, 61, size=10).tolist()
    out = []
    for i, n in enumerate(lens):
        s = "".join(pool[j % len(pool)] for j in range(i, i + 4))
        s = s[:n] if i % 3 else "".join(letters[int(c)] for c in rng.integers(0, len(letters), size=n))
        out.append(s)
    assert len(out) == 12 and {len(s) for s in out} >= {5, 60} and all(5 <= len(s) <= 60 for s in out)
    return out


def _score_setup(name, lag, net, dev):
    """Counters of the train and the reference strings, the RefModel, and the two AR functions the paths are compared through: a
    closure that forms the rows with kernels.ref_prior_rows from the codes (the same rows: bits must be equal), and a closure of
    plain torch ops (``_counts_to_probs``, the mix, + eps: rounding apart)."""
    import torch
    from bear_amd import ar_funcs, bear_ref, get_var_probs, kernels
    train, ref = (PROT_TRAIN, PROT_REF) if name == "prot" else (DNA_TRAIN, DNA_REF)
    counter = get_var_probs.DeviceCounter.from_sequences(train, lag, reverse=False, alphabet_name=name)
    ref_counter = get_var_probs.DeviceCounter.from_sequences(ref, lag, reverse=False, alphabet_name=name)
    W = counter.width
    net_func = None
    if net == "lin":
        net_func, _ = ar_funcs.make_ar_func_linear(lag, W - 1, device=dev, generator=torch.Generator(device=dev).manual_seed(lag))
    model = get_var_probs.RefModel(lag, name, HS[0], 0.2, 0.3, net_func)
    bits, rank = kernels.SCORE_BITS[W], torch.from_numpy(counter.rank.astype(np.int64)).to(dev)

    def keys_of_codes(codes):                                  # codes_of_keys' inverse
        sym = torch.where(codes.long() == W - 1, W, codes.long())
        shifts = torch.arange(lag - 1, -1, -1, dtype=torch.int64, device=dev) * bits
        return (rank[sym] << shifts[None, :]).sum(1)

    def rows_kernel(codes):
        return kernels.ref_prior_rows(ref_counter.keys, ref_counter.counts_by_key, keys_of_codes(codes), model.net_rows(codes), model.tau,
                                      model.net_weight)

    def rows_torch(codes):
        g_rows = model.net_rows(codes)
        if g_rows is None:
            g_rows = torch.zeros((codes.shape[0], W), dtype=torch.float64, device=dev)
            g_rows[:, -1] = 1.0
        ref_in = bear_ref._ref_input(ref_counter.rows_of_keys(keys_of_codes(codes)))
        jc = bear_ref._counts_to_probs(ref_in, torch.tensor(model.tau, dtype=torch.float64, device=dev), W - 1)
        return (model.net_weight * g_rows + jc) / (model.net_weight + 1) + EPS
    return counter, ref_counter, model, rows_kernel, rows_torch


@pytest.mark.parametrize("name,lag,net", [("dna", 1, "stop"), ("dna", 5, "stop"), ("prot", 1, "stop"), ("prot", 5, "stop"), ("prot", 5, "lin")],
                         ids=lambda v: str(v))
def test_scoring_equals_the_existing_device_path(name, lag, net, dev, monkeypatch):
    """get_bear_probs (sampled with a seed, MAP) and get_bear_probs_seqs (sampled, MAP, the exact marginal on the device) with
    ref_model= / ref_counter=: bit for bit what the existing device path gives when its AR function forms the same rows, and, to
    the figures tests/test_score_gpu.py (rtol = atol = 1e-12) and tests/test_marg_gpu.py (1e-11) hold the device to against the
    host, what it gives on rows formed by plain torch ops."""
    from bear_amd import get_var_probs
    counter, ref_counter, model, rows_kernel, rows_torch = _score_setup(name, lag, net, dev)
    rng = np.random.default_rng(17 + lag)
    vars_, seqs = _variants(name, rng), _sequences(name, rng)
    assert len(WT[name]) == 40 and len(vars_) == 30
    ref_kw = dict(ref_model=model, ref_counter=ref_counter)
    calls = {
        "vars": lambda bp, **kw: get_var_probs.get_bear_probs(bp, WT[name], vars_, 0, mc_samples=5, vans=VANS, h=HS, seed=9, counter=counter, **kw),
        "vars_map": lambda bp, **kw: get_var_probs.get_bear_probs(bp, WT[name], vars_, 0, vans=VANS, h=HS, get_map=True, counter=counter, **kw),
        "seqs": lambda bp, **kw: get_var_probs.get_bear_probs_seqs(bp, seqs, 0, mc_samples=5, vans=VANS, h=HS, seed=9, counter=counter, **kw),
        "seqs_map": lambda bp, **kw: get_var_probs.get_bear_probs_seqs(bp, seqs, 0, vans=VANS, h=HS, get_map=True, counter=counter, **kw),
        "seqs_marg": lambda bp, **kw: get_var_probs.get_bear_probs_seqs(bp, seqs, 0, vans=VANS, h=HS, get_marg=True, marg_on_device=True,
                                                                       counter=counter, **kw),
    }
    shapes = {"vars": (30, 5, 5), "vars_map": (30, 6), "seqs": (12, 5, 5), "seqs_map": (12, 6), "seqs_marg": (12, 5)}
    got = {k: f(None, **ref_kw) for k, f in calls.items()}
    for rows, exact in ((rows_kernel, True), (rows_torch, False)):
        # the existing path: a folder whose AR function is `rows` (load_bear is the one thing replaced)
        monkeypatch.setattr(get_var_probs, "load_bear", lambda path, rows=rows: (lag, name, HS[0], rows, None))
        for k, f in calls.items():
            want = f("a folder")
            assert got[k].shape == want.shape == shapes[k] and np.isfinite(got[k]).all(), k
            if exact:
                assert np.array_equal(got[k], want), (k, float(np.abs(got[k] - want).max()))
            elif k == "seqs_marg":
                print(name, lag, net, k, "largest |difference| / |score|", float((np.abs(got[k] - want) / np.abs(want)).max()))
                assert np.all(np.abs(got[k] - want) <= 1e-11 * np.abs(want)), k
            else:
                print(name, lag, net, k, "largest |difference|", float(np.abs(got[k] - want).max()))
                assert np.allclose(got[k], want, rtol=1e-12, atol=1e-12), k
    assert np.abs(got["vars_map"]).max() > 0.01 and np.abs(got["seqs_marg"]).min() > 1.0
    # the default h is the model's
    one = get_var_probs.get_bear_probs(None, WT[name], vars_, 0, vans=VANS, get_map=True, counter=counter, **ref_kw)
    assert one.shape == (30, 5) and np.array_equal(one[:, 0], got["vars_map"][:, 0])


# ------------------------------------------------------------------------------------------- generation
def run_ref_case(case, dev, cuts=(L,), stepwise=False, n_seq=37, sample=None):
    """A case of test_ref_score_cpu.REF_CASES through kernels.generate_whole_ref, ``sum(cuts)`` steps cut into launches of ``cuts``
    steps -> a dict of FIELDS as NumPy arrays.  ``stepwise``: one step per launch on the net function's rows (the one-hot at the
    stop, kernels.linear_forward_wide), as assemble.generate_sequences does."""
    import torch
    from bear_amd import kernels
    name, lag, net, model = case
    inputs = r.ref_case_inputs(case)
    W, rank, n_steps = inputs["W"], inputs["rank"], sum(cuts)
    starts = w.start_keys(n_seq, rank, lag)
    keys, sample = _i64(starts, dev), _i64(inputs["sample"][:n_seq] if sample is None else sample, dev)
    left = torch.full((n_seq,), n_steps, dtype=torch.int32, device=dev)
    length = torch.zeros(n_seq, dtype=torch.int32, device=dev)
    stopped = torch.zeros(n_seq, dtype=torch.uint8, device=dev)
    letters = torch.full((n_seq, n_steps), 0xFF, dtype=torch.uint8, device=dev)
    codes = torch.from_numpy(g.unpack_codes(starts, rank, W, lag)).to(dev) if stepwise else torch.full((n_seq, lag), -9, dtype=torch.int8, device=dev)
    args = (_i64(inputs["table"], dev), _counts(inputs["counts"], dev), _i64(inputs["ref_table"], dev), _counts(inputs["ref_counts"], dev), rank,
            lag, keys, sample, left, length, stopped, letters)
    kw = dict(h=inputs["h"]) if "h" in inputs else dict(get_map=True)
    mat = torch.from_numpy(inputs["mat"].copy()).to(dev) if inputs["mat"] is not None else None
    if stepwise:
        stop_rows = torch.zeros((n_seq, W), dtype=torch.float64, device=dev)
        stop_rows[:, -1] = 1.0
        for t in range(n_steps):
            rows = stop_rows if mat is None else kernels.linear_forward_wide(codes, mat, lag)
            kernels.generate_whole_ref(*args, t, 1, inputs["seed"], inputs["tau"], inputs["nw"], net_rows=rows, codes=codes, **kw)
    else:
        step0 = 0
        for n in cuts:
            kernels.generate_whole_ref(*args, step0, n, inputs["seed"], inputs["tau"], inputs["nw"], mat=mat, codes=codes, **kw)
            step0 += n
    out = dict(letters=letters, keys=keys, left=left, length=length, stopped=stopped, codes=codes)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["keys"] = out["keys"].view(np.uint64)
    return out


def assert_equals_replica(got, want, case, n=None):
    inputs = r.ref_case_inputs(case)
    differ = np.flatnonzero((got["letters"][:n] != want["letters"]).any(axis=1))
    assert differ.size == 0, (case, "sequences that differ", differ.tolist(), "smallest gap of the case", want["gap"])
    for name in ("keys", "left", "length", "stopped"):
        assert np.array_equal(got[name][:n], want[name]), (case, name)
    assert np.array_equal(got["codes"][:n], g.unpack_codes(want["keys"], inputs["rank"], inputs["W"], inputs["lag"])), case


def assert_same_bytes(a, b, what):
    for name in FIELDS:
        assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (what, name)


@pytest.mark.parametrize("n_seq", r.N_SEQS)
@pytest.mark.parametrize("case", r.REF_CASES, ids=r.REF_CASE_IDS)
def test_bytes_equal_the_replica(case, n_seq, dev):
    assert_equals_replica(run_ref_case(case, dev, n_seq=n_seq), r.ref_expected(case, n_seq), case)


@pytest.mark.parametrize("case", r.REF_CASES, ids=r.REF_CASE_IDS)
def test_one_launch_equals_stepwise_and_any_cut(case, dev):
    whole = run_ref_case(case, dev)
    assert_same_bytes(whole, run_ref_case(case, dev, stepwise=True), "stepwise")
    for cuts in ((13, 35), (48, 0), (0, 7, 41)):
        assert_same_bytes(whole, run_ref_case(case, dev, cuts), cuts)
    assert_equals_replica(whole, r.ref_expected(case, 37), case)


def test_a_sequence_is_the_same_wherever_it_sits(dev):
    """4097 sequences of the linear case, whose grid is capped at 512 blocks of 8: sequence i carries the sample index of sequence
    i % 37 and must equal it on the second trip of the grid-stride loop; the first 37 are the replica's."""
    case, n_seq, steps = r.REF_CASES[4], 4097, 4
    sample = r.ref_case_inputs(case)["sample"][np.arange(n_seq) % 37]
    got = run_ref_case(case, dev, cuts=(steps,), n_seq=n_seq, sample=sample)
    for name in FIELDS:
        assert np.array_equal(got[name], got[name][:37][np.arange(n_seq) % 37]), name
    want = r.run_ref_replica(case, n_steps=steps, n_seq=37)
    assert want["gap"] > g.MIN_GAP
    assert_equals_replica(got, want, case, n=37)


_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/oracle"]
import numpy as np
import torch
from bear_amd import _lib
import test_ref_score_gpu as t
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
np.save(sys.argv[2], np.frombuffer(t.det_bytes(torch.device("cuda", 0)), dtype=np.uint8))
"""


def det_bytes(dev):
    return b"".join(run_ref_case(case, dev)[name].tobytes() for case in r.REF_CASES for name in FIELDS)


def test_deterministic_library_gives_the_same_bytes(dev, tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    here = det_bytes(dev)
    script = tmp_path / "det_ref_generate.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, str(script), ROOT, str(tmp_path / "det.npy")], env=env,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert np.load(tmp_path / "det.npy").tobytes() == here


# ------------------------------------------------------------------------------------------- assemble.generate_sequences
def _count_launches(monkeypatch):
    from bear_amd import kernels
    calls = []
    launch = kernels._launch
    monkeypatch.setattr(kernels, "_launch", lambda device, name, *a: (calls.append(name), launch(device, name, *a))[1])
    return calls


def _replica_strings(counter, ref_counter, model, num, max_len, seed, h=None, get_map=False, net=None):
    """generate_sequences' answer from the replica over the counters' own tables (the empty prompt)."""
    name, lag = counter.alphabet_name, counter.lag
    rank = g.ranks(name)
    table, counts = counter.keys.cpu().numpy().view(np.uint64), counter.counts_by_key.cpu().numpy()
    ref_table, ref_counts = ref_counter.keys.cpu().numpy().view(np.uint64), ref_counter.counts_by_key.cpu().numpy()
    prior = r.per_distinct_key(lambda keys: r.ref_rows_replica(keys, ref_table, ref_counts, net, model.tau, model.net_weight))
    strings, stopped, gap = w.replica_strings(table, counts, name, lag, w.start_keys(num, rank, lag), np.arange(num), max_len, seed, prior=prior,
                                              **(dict(get_map=True) if get_map else dict(h=model.h if h is None else h)))
    assert gap > g.MIN_GAP, gap
    return np.array(strings, dtype=str).reshape(1, num), stopped.reshape(1, num)


def _write_folder(path, name, lag, net_name, params):
    """A model folder as models/train_bear_ref.py leaves it (config.cfg + results.pickle), its data the bundled test table."""
    import pickle
    config = configparser.ConfigParser()
    config.read(os.path.join(ROOT, "bear_amd", "models", "config_files", "bear_stop_bear.cfg"))
    config["data"]["alphabet"], config["hyperp"]["lag"], config["model"]["ar_func_name"] = name, str(lag), net_name
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.cfg"), "w") as f:
        config.write(f)
    with open(os.path.join(path, "results.pickle"), "wb") as f:
        pickle.dump({"params": params}, f)


def test_generate_sequences_with_a_reference_model(dev, tmp_path, monkeypatch):
    """The stop net function: one launch by default, the replica's strings; ``stepwise`` the same strings in a launch per step; a
    folder as ref_model=; get_map generates at the AR function's MAP value."""
    from bear_amd import assemble, get_var_probs
    counter = get_var_probs.DeviceCounter.from_sequences(DNA_TRAIN, 5, reverse=False, alphabet_name="dna")
    ref_counter = get_var_probs.DeviceCounter.from_sequences(DNA_REF, 5, reverse=False, alphabet_name="dna")
    folder = str(tmp_path / "model")
    _write_folder(folder, "dna", 5, "stop", [np.array(math.log(0.5)), np.array(math.log(0.25)), np.array(math.log(0.05))])
    model, data, ds_loc, ds_loc_ref = get_var_probs.load_bear_ref(folder)
    assert (model.lag, model.alphabet, model.net_func, ds_loc, ds_loc_ref) == (5, "dna", None, 0, 2) and data.counts.shape[0] == 3
    assert (model.h, model.tau, model.net_weight) == (math.exp(math.log(0.5)), math.exp(math.log(0.25)), math.exp(math.log(0.05)))
    calls = _count_launches(monkeypatch)
    num, max_len = 40, 30
    one, s_one = assemble.generate_sequences(counter, num, max_len, ref_model=folder, ref_counter=ref_counter, seed=11)
    assert calls.count("bear_generate_whole_ref_f64") == 1 and "bear_generate_whole_f64" not in calls and "bear_ref_prior_rows_f64" not in calls
    want, want_stopped = _replica_strings(counter, ref_counter, model, num, max_len, 11)
    assert np.array_equal(one, want) and np.array_equal(s_one, want_stopped)
    assert s_one.any() and len(set(one[0].tolist())) > num // 2 and set("".join(one[0])) <= set("ACGT")
    del calls[:]
    steps, s_steps = assemble.generate_sequences(counter, num, max_len, ref_model=model, ref_counter=ref_counter, seed=11, stepwise=True)
    assert 1 < calls.count("bear_generate_whole_ref_f64") <= max_len
    assert np.array_equal(one, steps) and np.array_equal(s_one, s_steps)
    m, s_m = assemble.generate_sequences(counter, num, max_len, ref_model=model, ref_counter=ref_counter, seed=11, get_map=True, h=2.0)
    want, want_stopped = _replica_strings(counter, ref_counter, model, num, max_len, 11, get_map=True)
    assert np.array_equal(m, want) and np.array_equal(s_m, want_stopped)
    # a folder trained by bear_net: its parameter list has no tau_signed / net_weight_signed
    _write_folder(str(tmp_path / "net"), "dna", 5, "stop", [np.array(0.0)])
    with pytest.raises(ValueError, match="bear_net"):
        get_var_probs.load_bear_ref(str(tmp_path / "net"))
    _write_folder(str(tmp_path / "net_lin"), "dna", 5, "linear", [np.array(0.0), np.zeros((5, 5, 5))])
    with pytest.raises(ValueError, match="bear_net"):
        get_var_probs.load_bear_ref(str(tmp_path / "net_lin"))


def test_generate_sequences_with_a_linear_net_function(dev, monkeypatch):
    """The protein linear net function: one launch (the function and the mixing inside the kernel), the replica's strings, and the
    same strings stepwise on kernels.linear_forward_wide rows."""
    import torch
    from bear_amd import ar_funcs, assemble, get_var_probs
    lag = 3
    counter = get_var_probs.DeviceCounter.from_sequences(PROT_TRAIN, lag, reverse=False, alphabet_name="prot")
    ref_counter = get_var_probs.DeviceCounter.from_sequences(PROT_REF, lag, reverse=False, alphabet_name="prot")
    net_func, params = ar_funcs.make_ar_func_linear(lag, 20, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    with torch.no_grad():
        params[0].mul_(20.0)                                   # a net function with something to say
    model = get_var_probs.RefModel(lag, "prot", 0.5, 0.2, 3.0, net_func)
    calls = _count_launches(monkeypatch)
    num, max_len = 30, 40
    one, s_one = assemble.generate_sequences(counter, num, max_len, ref_model=model, ref_counter=ref_counter, seed=8)
    assert calls.count("bear_generate_whole_ref_f64") == 1 and "bear_linear_forward_wide_f64" not in calls
    del calls[:]
    steps, s_steps = assemble.generate_sequences(counter, num, max_len, ref_model=model, ref_counter=ref_counter, seed=8, stepwise=True)
    n = calls.count("bear_generate_whole_ref_f64")
    assert 1 < n <= max_len and calls.count("bear_linear_forward_wide_f64") == n
    assert np.array_equal(one, steps) and np.array_equal(s_one, s_steps)
    mat = net_func.linear_mat.detach().cpu().numpy()
    want, want_stopped = _replica_strings(counter, ref_counter, model, num, max_len, 8,
                                          net=lambda keys: w.linear_rows(keys, mat, g.ranks("prot"), lag))
    assert np.array_equal(one, want) and np.array_equal(s_one, want_stopped)


def test_train_then_use_round_trip(dev, tmp_path):
    """bear_stop_bear.cfg shortened to 20 steps, trained into tmp_path; load_bear_ref; counters of the train and the reference
    column of its own table; ten substitutions scored, 8 sequences of at most 30 letters generated: finite scores, and the
    replica's strings with the loaded tau, nw and h."""
    import torch
    from bear_amd import assemble, get_var_probs
    from bear_amd.models import train_bear_ref
    config = configparser.ConfigParser()
    config.read(os.path.join(ROOT, "bear_amd", "models", "config_files", "bear_stop_bear.cfg"))
    folder = str(tmp_path / "run")
    config["general"]["out_folder"] = folder + "*"
    config["train"]["epochs"] = "20s"
    config["test"]["test"], config["test"]["train_test"] = "False", "False"
    train_bear_ref.main(config)
    model, data, ds_loc, ds_loc_ref = get_var_probs.load_bear_ref(folder)
    assert (model.lag, model.alphabet, ds_loc, ds_loc_ref) == (5, "dna", 0, 2) and model.net_func is None
    start = (1.0, 1 / 30, 0.01)                                # bear_ref's initial h, tau, nw: 20 Adam steps moved all three
    assert all(v > 0 and math.isfinite(v) and abs(math.log(v / s)) > 1e-3 for v, s in zip((model.h, model.tau, model.net_weight), start))
    counter = get_var_probs.DeviceCounter.from_dataset(data, ds_loc)
    ref_counter = get_var_probs.DeviceCounter.from_dataset(data, ds_loc_ref)
    wt = WT["dna"]
    vars_ = [f"{wt[p]}{p}{'ACGT'[('ACGT'.index(wt[p]) + 1 + p % 3) % 4]}" for p in (0, 3, 7, 11, 16, 20, 25, 31, 36, 39)]
    scores = get_var_probs.get_bear_probs(None, wt, vars_, 0, mc_samples=5, seed=2, counter=counter, ref_model=folder, ref_counter=ref_counter)
    assert scores.shape == (10, 4, 5) and np.isfinite(scores).all() and np.abs(scores).max() > 0
    seqs, stopped = assemble.generate_sequences(counter, 8, 30, ref_model=folder, ref_counter=ref_counter, seed=5)
    want, want_stopped = _replica_strings(counter, ref_counter, model, 8, 30, 5)
    assert np.array_equal(seqs, want) and np.array_equal(stopped, want_stopped)
    assert set("".join(seqs[0])) <= set("ACGT") and max(len(s) for s in seqs[0]) > 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(dev, monkeypatch):
    import torch
    from bear_amd import assemble, get_var_probs, kernels
    counter = get_var_probs.DeviceCounter.from_sequences(DNA_TRAIN, 3, reverse=False, alphabet_name="dna")
    ref_counter = get_var_probs.DeviceCounter.from_sequences(DNA_REF, 3, reverse=False, alphabet_name="dna")
    ref_no_end = get_var_probs.DeviceCounter.from_sequences(DNA_REF, 3, reverse=False, no_end=True, alphabet_name="dna")
    ref_lag4 = get_var_probs.DeviceCounter.from_sequences(DNA_REF, 4, reverse=False, alphabet_name="dna")
    prot = get_var_probs.DeviceCounter.from_sequences(PROT_REF, 3, reverse=False, alphabet_name="prot")
    host = get_var_probs.make_sequence_counter(DNA_TRAIN, 3, reverse=False)
    model = get_var_probs.RefModel(3, "dna", 0.5, 0.2, 0.3)
    _ = counter.counts_by_key, ref_counter.counts_by_key, ref_lag4.counts_by_key, prot.counts_by_key

    def no_launch(*a):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(kernels, "_launch", no_launch)
    wt, vars_, seqs = WT["dna"], ["A0T"], ["ACGTACGT"]
    entries = [lambda **kw: get_var_probs.get_bear_probs(kw.pop("bear_path", None), wt, vars_, 0, counter=kw.pop("counter", counter), **kw),
               lambda **kw: get_var_probs.get_bear_probs_seqs(kw.pop("bear_path", None), seqs, 0, counter=kw.pop("counter", counter), **kw),
               lambda **kw: assemble.generate_sequences(kw.pop("counter", counter), 2, 5, seed=1, **kw)]
    for call in entries:
        with pytest.raises(ValueError, match="go together"):
            call(ref_model=model)
        with pytest.raises(ValueError, match="go together"):
            call(ref_counter=ref_counter)
        with pytest.raises(ValueError, match="no_end"):
            call(ref_model=model, ref_counter=ref_no_end)
        with pytest.raises(ValueError, match="lag-4"):
            call(ref_model=model, ref_counter=ref_lag4)
        with pytest.raises(ValueError, match="'prot'"):
            call(ref_model=model, ref_counter=prot)
        with pytest.raises(ValueError, match="lag-3"):
            call(ref_model=get_var_probs.RefModel(4, "dna", 0.5, 0.2, 0.3), ref_counter=ref_counter)
        with pytest.raises(ValueError, match="bear_path"):
            call(ref_model=model, ref_counter=ref_counter, bear_path="a folder")
    for call in entries[:2]:
        with pytest.raises(ValueError, match="DeviceCounter"):
            call(ref_model=model, ref_counter=ref_counter, counter=host)
        with pytest.raises(ValueError, match="DeviceCounter"):
            call(ref_model=model, ref_counter=host)
    with pytest.raises(ValueError, match="marg_on_device"):
        get_var_probs.get_bear_probs_seqs(None, seqs, 0, counter=counter, get_marg=True, ref_model=model, ref_counter=ref_counter)
    with pytest.raises(ValueError, match="ar_func"):
        assemble.generate_sequences(counter, 2, 5, seed=1, ref_model=model, ref_counter=ref_counter, ar_func=lambda codes: None, h=1.0)
    with pytest.raises(ValueError, match="van"):
        assemble.generate_sequences(counter, 2, 5, seed=1, ref_model=model, ref_counter=ref_counter, van=0.5)
    for bad in (dict(h=0.0), dict(tau=0.0), dict(net_weight=float("nan")), dict(lag=0), dict(alphabet="abc")):
        with pytest.raises(ValueError):
            get_var_probs.RefModel(**{**dict(lag=3, alphabet="dna", h=0.5, tau=0.2, net_weight=0.3), **bad})
    # the wrappers
    query = torch.zeros(4, dtype=torch.int64, device=dev)
    net = torch.full((4, 5), 0.2, dtype=torch.float64, device=dev)
    ok = (ref_counter.keys, ref_counter.counts_by_key, query, None, 0.2, 0.3)
    for i, bad in ((0, ref_counter.keys.int()), (1, ref_counter.counts_by_key[:-1]), (1, ref_counter.counts_by_key[:, :4].contiguous()),
                   (2, query.int()), (3, net[:3]), (3, net.float()), (4, 0.0), (4, float("inf")), (5, -1.0), (5, float("nan"))):
        a = list(ok)
        a[i] = bad
        with pytest.raises(ValueError):
            kernels.ref_prior_rows(*a)
    with pytest.raises(ValueError):
        kernels.ref_prior_rows(ref_counter.keys[:0], None, query, None, 0.2, 0.3)             # an empty table needs width=
    with pytest.raises(ValueError):
        kernels.ref_prior_rows(*ok, eps=-1.0)
    n, lag = 6, 3
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    sample = torch.arange(n, dtype=torch.int64, device=dev)
    left = torch.full((n,), 4, dtype=torch.int32, device=dev)
    length = torch.zeros(n, dtype=torch.int32, device=dev)
    stopped = torch.zeros(n, dtype=torch.uint8, device=dev)
    letters = torch.full((n, 4), 0xFF, dtype=torch.uint8, device=dev)
    rows = torch.full((n, 5), 0.2, dtype=torch.float64, device=dev)
    mat = torch.zeros((lag, 21, 21), dtype=torch.float64, device=dev)
    a = [counter.keys, counter.counts_by_key, ref_counter.keys, ref_counter.counts_by_key, counter.rank, lag, keys, sample, left, length, stopped,
         letters]
    for bad in (dict(n_steps=4), dict(n_steps=4, h=0.0), dict(n_steps=2, net_rows=rows, h=1.0), dict(n_steps=1, net_rows=rows[:5], h=1.0),
                dict(n_steps=4, mat=mat, h=1.0), dict(n_steps=1, net_rows=rows, mat=mat, h=1.0), dict(n_steps=4, h=1.0, tau=0.0),
                dict(n_steps=4, h=1.0, net_weight=float("inf")), dict(n_steps=4, h=1.0, eps=float("nan")), dict(n_steps=5, h=1.0),
                dict(n_steps=4, h=1.0, ref_counts=ref_counter.counts_by_key[:-1]), dict(n_steps=4, h=1.0, ref_table=ref_counter.keys.int())):
        kw = dict(bad)
        b = list(a)
        b[2], b[3] = kw.pop("ref_table", a[2]), kw.pop("ref_counts", a[3])
        with pytest.raises(ValueError):
            kernels.generate_whole_ref(*b, 0, kw.pop("n_steps"), 1, kw.pop("tau", 0.2), kw.pop("net_weight", 0.3), **kw)
