"""GPU tests of sequence generation on the device (bear_generate_steps_f64, kernels_generate.h; assemble.assemble_no_ends with a
DeviceCounter).  The letters are held to the NumPy replica of tests/test_generate_cpu.py and must EQUAL it: that file shows that
every step of these cases is decided by a margin no rounding difference between host and device reaches."""
import configparser
import os
import subprocess
import sys

import numpy as np
import pytest

import test_generate_cpu as g
from conftest import ROOT

pytestmark = pytest.mark.gpu

L = int(g.LENGTHS.max())


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _i64(a, dev):
    import torch
    return torch.from_numpy(np.array(a).view(np.int64)).to(dev)


def run_case(case, dev, cuts=(L,)):
    """A case of test_generate_cpu.CASES through kernels.generate_steps, the steps cut into launches of ``cuts`` steps (a model with
    prior rows: always one step per launch) -> ``(letters, keys uint64, left, codes)`` as NumPy arrays."""
    import torch
    from bear_amd import kernels
    alphabet_name, lag, model, kind = case
    inputs = g.expected(case)[0]
    W, rank = inputs["W"], g.ranks(alphabet_name)
    table, counts = _i64(inputs["table"], dev), torch.from_numpy(inputs["counts"].copy()).to(dev)
    keys, sample = _i64(inputs["starts"], dev), _i64(inputs["sample"], dev)
    left = torch.from_numpy(g.LENGTHS.astype(np.int32)).to(dev)
    letters = torch.full((g.N_SEQ, L), 0xFF, dtype=torch.uint8, device=dev)
    codes = torch.full((g.N_SEQ, lag), -9, dtype=torch.int8, device=dev)
    kw = g.model_args(model, W)
    prior = kw.pop("prior", None)
    if prior is None:
        assert sum(cuts) == L
        step0 = 0
        for n in cuts:
            kernels.generate_steps(table, counts, rank, lag, keys, sample, left, letters, step0, n, inputs["seed"], codes=codes, **kw)
            step0 += n
    else:
        for t in range(L):
            rows = torch.from_numpy(prior(keys.cpu().numpy().view(np.uint64))).to(dev)
            kernels.generate_steps(table, counts, rank, lag, keys, sample, left, letters, t, 1, inputs["seed"], prior=rows, codes=codes,
                                   **kw)
    return letters.cpu().numpy(), keys.cpu().numpy().view(np.uint64), left.cpu().numpy(), codes.cpu().numpy()


@pytest.mark.parametrize("case", g.CASES, ids=g.CASE_IDS)
def test_letters_equal_the_replica(case, dev):
    alphabet_name, lag, model, kind = case
    inputs, want_letters, want_keys, want_left, gap = g.expected(case)
    letters, keys, left, codes = run_case(case, dev)
    differ = np.flatnonzero((letters != want_letters).any(axis=1))
    assert differ.size == 0, (case, "sequences that differ", differ.tolist(), "smallest gap of the case", gap)
    assert np.array_equal(keys, want_keys) and np.array_equal(left, want_left) and not left.any()
    assert np.array_equal(codes, g.unpack_codes(want_keys, g.ranks(alphabet_name), inputs["W"], lag))


@pytest.mark.parametrize("case", [("dna", 5, "bmm", "trained"), ("prot", 12, "bmm", "trained"), ("prot", 5, "bmm_map", "trained")],
                         ids=lambda c: "-".join(map(str, c)))
def test_any_cut_of_the_steps_gives_the_same_letters(case, dev):
    whole = run_case(case, dev)
    for cuts in ((13, L - 13), (1,) * L, (L, 0), (0, 7, L - 7)):
        parts = run_case(case, dev, cuts)
        for a, b in zip(whole, parts):
            assert np.array_equal(a, b), cuts
    assert np.array_equal(whole[0], g.expected(case)[1])


DET_CASES = [("dna", 21, "bmm", "trained"), ("prot", 5, "bear", "trained"), ("prot", 12, "bmm", "trained"), ("dna", 5, "ar_map", "trained")]

_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/oracle"]
import numpy as np
import torch
from bear_amd import _lib
import test_generate_gpu as t
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
np.save(sys.argv[2], np.stack([t.run_case(case, torch.device("cuda", 0))[0] for case in t.DET_CASES]))
"""


def test_deterministic_library_gives_the_same_letters(dev, tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    here = np.stack([run_case(case, dev)[0] for case in DET_CASES])
    script = tmp_path / "det_generate.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npy")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    there = np.load(tmp_path / "det.npy")
    assert there.shape == here.shape and there.tobytes() == here.tobytes()


# ------------------------------------------------------------------------------------------- assemble_no_ends
def _write_seeds(path, seeds):
    path.write_text("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seeds)))
    return str(path)


def test_assemble_bmm_on_the_device(dev, tmp_path, monkeypatch):
    """test_assemble_gpu.py::test_assemble_bmm with the table left on the device: the periodic continuation, zero entropies, the
    files -- and what only this path promises: the same strings for the same seed, whatever the batch size, in one launch a flank."""
    from bear_amd import assemble, get_var_probs, kernels
    counter = get_var_probs.DeviceCounter.from_sequences(["ACGT" * 50] * 40, 3, reverse=False, no_end=True)
    seeds = _write_seeds(tmp_path / "seeds.fa", ["ACGTACG", "GTACGTA"])
    calls = []
    launch = kernels._launch
    monkeypatch.setattr(kernels, "_launch", lambda device, name, *a: (calls.append(name), launch(device, name, *a))[1])
    kw = dict(van=0.01, lag=3, alphabet_name="dna", counter=counter, seed=3)
    gen, ent = assemble.assemble_no_ends(seeds, [[0, 12], [4, 8]], 5, None, None, save_folder=str(tmp_path / "out"), **kw)
    assert calls.count("bear_generate_steps_f64") == 2 and "bear_logdir_sample_f64" not in calls      # one launch per direction
    assert gen.shape == (2, 5) and len(ent) == 2
    for s in gen[0]:
        assert s == "ACGTACG" + "TACGTACGTACG"
    for s in gen[1]:
        assert len(s) == 4 + 7 + 8 and s[4:11] == "GTACGTA" and s[11:] == "CGTACGTA" and s[:4] == "GTAC"
    assert (tmp_path / "out" / "seqs.fa").read_text().count(">") == 10
    assert ent[0].shape == (19,) and ent[1].shape == (19,) and np.all(ent[0] == 0.0) and np.all(ent[1] == 0.0)
    # a table with something to choose: same seed, same strings; the batch size is nothing to the device path; another seed differs
    counter = get_var_probs.DeviceCounter.from_sequences(["ACGTTGCAAGTCCATG" * 4, "GGATCCAATTGACT" * 3], 3, reverse=True, no_end=True)
    kw = dict(van=0.5, lag=3, alphabet_name="dna", counter=counter)
    a, _ = assemble.assemble_no_ends(seeds, [[9, 30], [17, 0]], 7, None, None, seed=11, **kw)
    b, _ = assemble.assemble_no_ends(seeds, [[9, 30], [17, 0]], 7, None, None, seed=11, batch_size=3, **kw)
    c, _ = assemble.assemble_no_ends(seeds, [[9, 30], [17, 0]], 7, None, None, seed=12, **kw)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert len(set(a[0].tolist())) > 1 and all(len(s) == 9 + 7 + 30 for s in a[0]) and all(len(s) == 17 + 7 for s in a[1])
    # ... and they are the replica's strings
    assert np.array_equal(a, _assemble_replica(counter, ["ACGTACG", "GTACGTA"], [[9, 30], [17, 0]], 7, 11, van=0.5))
    # device_path=False: the host loop, which draws from numpy's generator
    h, _ = assemble.assemble_no_ends(seeds, [[0, 6], [2, 3]], 2, None, None, seed=11, device_path=False, **kw)
    assert h.shape == (2, 2) and "bear_logdir_sample_f64" in calls


def _assemble_replica(counter, seeds, lengths, num_to_gen, seed, **model):
    """assemble_no_ends' strings from the replica: both directions, sample indices direction * n_total + seed * num_to_gen + replicate."""
    from bear_amd import assemble
    name, lag, W = counter.alphabet_name, counter.lag, counter.width
    rank = g.ranks(name)
    code = {ch: c for c, ch in enumerate(g.ALPHABETS[name])}
    table, counts = counter.keys.cpu().numpy().view(np.uint64), counter.counts_by_key.cpu().numpy()
    fwd = np.repeat(np.array(seeds), num_to_gen)
    lens = np.repeat(np.asarray(lengths).reshape(len(seeds), 2), num_to_gen, axis=0)
    n_total = len(fwd)
    flanks, gaps = [], []
    for d, seqs in enumerate(([assemble.reverse_complement(s) for s in fwd], fwd)):
        ends = g.pack(np.array([[code[ch] for ch in s[-lag:]] for s in seqs]), rank, W)
        letters = np.full((n_total, max(int(lens[:, d].max()), 1)), 0xFF, dtype=np.uint8)
        _, _, gap = g.replica(table, counts, rank, lag, ends, np.arange(n_total) + d * n_total, lens[:, d], 0, int(lens[:, d].max()),
                              seed, letters=letters, **model)
        gaps.append(gap)
        flanks.append(["".join(g.ALPHABETS[name][b] for b in row[:n]) for row, n in zip(letters, lens[:, d])])
    assert min(gaps) > g.MIN_GAP, gaps
    out = [assemble.reverse_complement(l) + s + r for l, r, s in zip(flanks[0], flanks[1], fwd)]
    return np.array(out).reshape(-1, num_to_gen)


def test_assemble_from_a_trained_model_folder(dev, tmp_path):
    """A folder as test_sampling_gpu.py::test_trained_model_folder_restart_and_variant_scores builds one (two epochs are enough
    here): the flanks grow through its AR function, one launch per step, and equal the replica fed the same prior rows."""
    import torch
    from bear_amd import assemble, get_var_probs
    from bear_amd.models import train_bear_net
    config = configparser.ConfigParser()
    config.read(os.path.join(ROOT, "bear_amd", "models", "config_files", "bear_lin_bear.cfg"))
    config["train"]["epochs"] = "2"
    config["train"]["batch_size"] = "1500"
    config["general"]["out_folder"] = str(tmp_path / "m1") + "*"
    config["test"]["test"] = "False"
    config["test"]["train_test"] = "False"
    assert train_bear_net.main(config) == 1
    folder = str(tmp_path / "m1")
    lag, alphabet, h, ar_func, data = get_var_probs.load_bear(folder)
    assert lag == 5 and alphabet == "dna"
    counter = get_var_probs.DeviceCounter.from_dataset(data, 0, no_end=True)
    seeds = ["ACGTACGTTAGC", "TTGACCA", "GGGGG"]
    lengths = [[3, 9], [0, 14], [11, 2]]
    path = _write_seeds(tmp_path / "seeds.fa", seeds)

    def prior(keys):
        codes = torch.from_numpy(g.unpack_codes(keys, g.ranks("dna"), 5, lag)).to(dev)
        return ar_func(codes).to(torch.float64).cpu().numpy()
    got, ent = assemble.assemble_no_ends(path, lengths, 4, folder, None, counter=counter, seed=21)
    assert got.shape == (3, 4) and len(ent) == 3
    assert np.array_equal(got, _assemble_replica(counter, seeds, lengths, 4, 21, prior=prior, h=h))
    got_map, _ = assemble.assemble_no_ends(path, lengths, 4, folder, None, counter=counter, seed=21, get_map=True)
    assert np.array_equal(got_map, _assemble_replica(counter, seeds, lengths, 4, 21, prior=prior, get_map=True))      # model 0: the AR model
    got_bmm, _ = assemble.assemble_no_ends(path, lengths, 4, folder, None, counter=counter, seed=21, van=0.3, lag=5, alphabet_name="dna")
    assert np.array_equal(got_bmm, _assemble_replica(counter, seeds, lengths, 4, 21, van=0.3))


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(dev, tmp_path, monkeypatch):
    import torch
    from bear_amd import _lib, assemble, get_var_probs, kernels
    dna = get_var_probs.DeviceCounter.from_sequences(["ACGTTGCAAGTC" * 3], 3, reverse=False, no_end=True)
    prot = get_var_probs.DeviceCounter.from_sequences(["MKVLAARNDCEQ" * 3], 2, reverse=False, no_end=True, alphabet_name="prot")
    n, lag, W = 6, 3, 5
    rank = kernels.score_ranks("dna")
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    sample = torch.arange(n, dtype=torch.int64, device=dev)
    left = torch.full((n,), 4, dtype=torch.int32, device=dev)
    letters = torch.full((n, 4), 0xFF, dtype=torch.uint8, device=dev)
    prior = torch.full((n, W), 0.2, dtype=torch.float64, device=dev)
    args = (dna.keys, dna.counts_by_key, rank, lag, keys, sample, left, letters)

    # the C entry, handed live pointers: every refusal of the header is BEAR_ERR_INVALID_ARG and nothing is written
    def entry(lag=lag, width=W, mode=0, get_map=0, h=1.0, van=1.0, prior=None, step0=0, n_steps=4, stride=4):
        p = kernels._ptr
        return _lib.lib().bear_generate_steps_f64(p(dna.keys), p(dna.counts_by_key), dna.keys.numel(), lag, width, rank.ctypes.data,
                                                  mode, get_map, h, van, p(prior), 1, p(keys), p(sample), p(left), n, step0, n_steps,
                                                  p(letters), stride, None, None)
    for bad in (dict(width=4), dict(lag=0), dict(lag=22), dict(mode=1, prior=prior, n_steps=2), dict(mode=1, n_steps=1),
                dict(mode=2, get_map=1, n_steps=1), dict(mode=1, prior=prior, n_steps=1, h=0.0), dict(van=0.0), dict(van=float("nan")),
                dict(step0=1, n_steps=4, stride=4), dict(mode=2, prior=prior, n_steps=1)):
        assert entry(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((letters == 0xFF).all()) and bool((left == 4).all()) and bool((keys == 0).all())

    def no_launch(*a):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(kernels, "_launch", no_launch)
    # the wrapper
    for bad in (dict(n_steps=5, van=1.0), dict(n_steps=2, prior=prior, h=1.0), dict(n_steps=1, prior=prior), dict(n_steps=1),
                dict(n_steps=1, prior=prior, h=0.0), dict(n_steps=1, van=0.0), dict(n_steps=1, van=1.0, lag=22),
                dict(n_steps=1, van=1.0, codes=torch.zeros((n, lag + 1), dtype=torch.int8, device=dev))):
        kw = dict(bad)
        a = list(args)
        a[3] = kw.pop("lag", lag)
        with pytest.raises(ValueError):
            kernels.generate_steps(*a, 0, kw.pop("n_steps"), 1, **kw)
    # assemble_no_ends
    seeds = _write_seeds(tmp_path / "seeds.fa", ["ACGTACG", "GT"])
    kw = dict(van=0.5, lag=3, alphabet_name="dna", counter=dna, seed=1)
    with pytest.raises(ValueError, match="shorter"):
        assemble.assemble_no_ends(seeds, [[0, 4], [0, 4]], 2, None, None, **kw)
    seeds = _write_seeds(tmp_path / "seeds2.fa", ["ACNTACG"])
    with pytest.raises(ValueError, match="'N'"):
        assemble.assemble_no_ends(seeds, [[0, 4]], 2, None, None, **kw)
    seeds = _write_seeds(tmp_path / "seeds3.fa", ["ACGTACG"])
    with pytest.raises(ValueError, match="lag"):
        assemble.assemble_no_ends(seeds, [[0, 4]], 2, None, None, **dict(kw, lag=4))
    with pytest.raises(ValueError, match="lag"):
        assemble.assemble_no_ends(seeds, [[0, 4]], 2, None, None, **dict(kw, lag=2, alphabet_name="prot", counter=dna))
    pseeds = _write_seeds(tmp_path / "pseeds.fa", ["MKVLA"])
    with pytest.raises(ValueError, match="reverse complement"):
        assemble.assemble_no_ends(pseeds, [[2, 4]], 2, None, None, van=0.5, lag=2, alphabet_name="prot", counter=prot, seed=1)
    monkeypatch.undo()
    gen, _ = assemble.assemble_no_ends(pseeds, [[0, 6]], 3, None, None, van=0.5, lag=2, alphabet_name="prot", counter=prot, seed=1)
    assert gen.shape == (1, 3) and all(len(s) == 11 and s[:5] == "MKVLA" and set(s) <= set(g.ALPHABETS["prot"]) for s in gen[0])
