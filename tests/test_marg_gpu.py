"""GPU tests of the exact sequence marginal on the device (kernels_marg.h, kernels.score_marg, get_bear_probs_seqs with
``marg_on_device``): the kernels against the closed form evaluated with mpmath at 50 digits, a segment's bits wherever it stands,
the deterministic library, and the public call against its default (host) path.

The bound everywhere: ``|got - want| <= 1e-11 * mass`` with ``mass`` the sum of |group term| + the sum of |cell term| of that
segment and model -- the relative figure ``evaluate_wide`` is held to (tests/test_prot_gpu.py, rtol=1e-11), taken of the L1 mass
because the two brackets of a k-mer's term cancel; two paths that both carry it agree within twice that.  The largest ratio
``|got - want| / mass`` observed on an MI355X is recorded in DESIGN.md 4.7 (printed here per case)."""
import os
import subprocess
import sys
from collections import Counter

import mpmath
import numpy as np
import pytest
import torch

from bear_amd import core, get_var_probs, kernels
from conftest import ROOT
from test_score_gpu import PROT_WT, SEQ_CASES, VANS, _prot_table_600

pytestmark = pytest.mark.gpu

RTOL = 1e-11
HS = np.array([0.05, 3.0, 1.0])
K = 37
# empty in front, one transition, a k-mer seen with several letters, empty in the middle, one (row, letter) 3000 times (beyond the
# product / Stirling switch of bear_dm_item at 16, and beyond one chunk), 70 000 transitions over 37 rows, a short one, empty last
LENS = [0, 1, 9, 0, 3000, 70_000, 41, 0]
MODELS = {(0, 3): [3, 4, 5], (2, 0): [0, 1], (3, 3): [0, 1, 2, 3, 4, 5]}      # columns of the reference's 3 + 3 models


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _kernel_case(W):
    """Text-order (rows, letters) of every segment of LENS, and the K count and prior rows."""
    assert 3000 > kernels.MARG_CHUNK > 41
    rng = np.random.default_rng(100 + W)
    train = np.where(rng.random((K, W)) < 0.5, rng.poisson(20.0, (K, W)), 0).astype(np.uint32)
    train[[3, 17]] = 0                                     # rows that are all zero
    train[5, ::2] = 4294967295                             # entries at the counter's limit
    train[6] = 4294967295
    prior = rng.dirichlet(np.full(W, 0.5), size=K) + 1e-7
    segments = []
    for n in LENS:
        if n == 1:
            rows, letters = np.array([3]), np.array([W - 1])
        elif n == 9:
            rows, letters = np.array([5, 5, 5, 5, 6, 6, 5, 2, 5]), np.array([0, 1, 0, W - 1, 2, 2, 1, 0, 0])
        elif n == 3000:
            rows, letters = np.full(n, 9), np.full(n, 2)
        else:
            rows, letters = rng.integers(0, K, n), rng.integers(0, W, n)
            u = rng.random(n)
            rows = np.where(u < 0.1, -1, rows)             # 10 % of the positions hold no transition (1 % by the row alone,
            letters = np.where((u < 0.09) | ((u >= 0.1) & (u < 0.11)), 0xFF, letters)      # another 1 % by the letter alone)
        segments.append((rows.astype(np.int32), letters.astype(np.uint8)))
    return segments, train, prior


def _score(segments, train, prior, H, V, W):
    rows = np.concatenate([r for r, _ in segments] + [np.zeros(0, np.int32)])
    letters = np.concatenate([b for _, b in segments] + [np.zeros(0, np.uint8)])
    seg = np.concatenate([[0], np.cumsum([len(r) for r, _ in segments])]).astype(np.int64)
    got = kernels.score_marg(_dev(rows), _dev(letters), _dev(seg), _dev(train.view(np.int32)), _dev(prior) if H else None,
                             HS[:H] if H else None, VANS[:V] if V else None)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (len(segments), H + V)
    return got.cpu().numpy()


def _closed_form(groups_of_segments, hs, vans, W):
    """(want, mass) float64 [n_seg, H + V] of the formula, written out: per segment a list of groups ``(c [W] integers, f [W] floats
    or None, {letter: q})``; per model ``a_j = f_j / h + c_j`` (BEAR) or ``van + c_j``, ``A = sum_j a_j``, ``n = sum_j q_j``, and the term
    ``lgamma(A) - lgamma(A + n) + sum_{q_j > 0} [lgamma(a_j + q_j) - lgamma(a_j)]``.  mass: the absolute values of those brackets."""
    H, M = len(hs), len(hs) + len(vans)
    want, mass = np.zeros((len(groups_of_segments), M)), np.zeros((len(groups_of_segments), M))
    with mpmath.workdps(50):
        lg, mpf = mpmath.loggamma, mpmath.mpf
        for s, groups in enumerate(groups_of_segments):
            for m in range(M):
                total, l1 = mpf(0), mpf(0)
                for c, f, q in groups:
                    if m < H:
                        a = [mpf(float(f[j])) / mpf(float(hs[m])) + int(c[j]) for j in range(W)]
                    else:
                        a = [mpf(float(vans[m - H])) + int(c[j]) for j in range(W)]
                    A, n = mpmath.fsum(a), sum(q.values())
                    terms = [lg(A) - lg(A + n)] + [lg(a[j] + qj) - lg(a[j]) for j, qj in q.items()]
                    total += mpmath.fsum(terms)
                    l1 += mpmath.fsum(abs(t) for t in terms)
                want[s, m], mass[s, m] = float(total), float(l1)
    return want, mass


def _check(got, want, mass, rtol, what):
    err = np.abs(got - want)
    ratio = float((err / np.where(mass > 0, mass, 1.0)).max())
    print(f"marg {what}: largest |got - want| / mass = {ratio:.3e} (bound {rtol:.0e})")
    assert np.all(err <= rtol * mass), (what, ratio)
    assert not got[mass == 0].any()                        # nothing to sum: exactly 0


@pytest.fixture(scope="module", params=[5, 21])
def kernel_case(request):
    """The case at one width and its closed form under all 3 + 3 models, computed once."""
    W = request.param
    segments, train, prior = _kernel_case(W)
    groups_of_segments = []
    for rows, letters in segments:
        groups = {}
        for r, b in zip(rows.tolist(), letters.tolist()):
            if r >= 0 and b < W:
                groups.setdefault(r, Counter())[b] += 1
        groups_of_segments.append([(train[r], prior[r], q) for r, q in groups.items()])
    assert len(groups_of_segments[5]) == K and len(groups_of_segments[2]) == 3 and groups_of_segments[4][0][2] == {2: 3000}
    want, mass = _closed_form(groups_of_segments, HS, VANS, W)
    return W, segments, train, prior, want, mass


@pytest.mark.parametrize("H,V", sorted(MODELS))
def test_kernel_against_the_closed_form(kernel_case, H, V):
    W, segments, train, prior, want, mass = kernel_case
    got = _score(segments, train, prior, H, V, W)
    cols = MODELS[(H, V)]
    _check(got, want[:, cols], mass[:, cols], RTOL, f"kernel W={W} H={H} V={V}")
    assert all(not got[i].any() for i, n in enumerate(LENS) if n == 0) and np.abs(got[5]).min() > 100
    assert np.array_equal(got, _score(segments, train, prior, H, V, W))                # the same call twice: equal bits


@pytest.mark.parametrize("which", [6, 2, 5])
def test_a_segment_scores_the_same_wherever_it_stands(kernel_case, which):
    W, segments, train, prior, _, _ = kernel_case
    whole = _score(segments, train, prior, 3, 3, W)
    alone = _score([segments[which]], train, prior, 3, 3, W)
    between = _score([segments[4], segments[1], segments[which], segments[6], segments[2]], train, prior, 3, 3, W)   # at offset 3001
    backwards = _score(segments[::-1], train, prior, 3, 3, W)
    assert np.abs(alone[0]).min() > 1
    for row in (whole[which], between[2], backwards[len(segments) - 1 - which]):
        assert row.tobytes() == alone[0].tobytes()
    assert np.array_equal(backwards[::-1], whole)


_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from bear_amd import _lib
import test_marg_gpu as t
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
segments, train, prior = t._kernel_case(21)
np.save(sys.argv[2], t._score(segments, train, prior, 3, 3, 21))
"""


def test_deterministic_library_returns_the_same_bytes(tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    segments, train, prior = _kernel_case(21)
    here = _score(segments, train, prior, 3, 3, 21)
    script = tmp_path / "det_marg.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npy")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    there = np.load(tmp_path / "det.npy")
    assert there.shape == here.shape and there.tobytes() == here.tobytes()


def test_edges_and_a_sort_key_that_does_not_fit(monkeypatch):
    train = torch.zeros((3, 5), dtype=torch.int32, device="cuda")
    none = torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.uint8, device="cuda")
    seg = torch.zeros(5, dtype=torch.int64, device="cuda")
    out = kernels.score_marg(*none, seg, train, None, None, VANS)
    assert out.shape == (4, 3) and not out.any()
    assert kernels.score_marg(*none, seg[:1], train, None, None, VANS).shape == (0, 3)
    with pytest.raises(ValueError):
        kernels.score_marg(*none, seg, train, None, [1.0], VANS)                      # a BEAR model without prior rows
    with pytest.raises(ValueError):
        kernels.score_marg(*none, seg, train, None, None, [1.0, 0.0])
    monkeypatch.setattr(kernels, "_check_seg", lambda seg, device: 2 ** 53)           # (segments x 4 rows x 256 letters = 2^63)
    with pytest.raises(ValueError, match="63 bits"):
        kernels.score_marg(*none, seg, train, None, None, VANS)


# ------------------------------------------------------------------------------------------- the public call
def _string_groups(strings, lag, alphabet_name, count_rows, prior_rows):
    """Per string the groups of ``_closed_form``: its k-mers with the letters that follow them inside the string."""
    letter = {str(b): j for j, b in enumerate(core.alphabets_en[alphabet_name])}
    out = []
    for s in strings:
        groups = {}
        for p in range(lag, len(s)):
            groups.setdefault(s[p - lag:p], Counter())[letter[s[p]]] += 1
        out.append([(count_rows[k], None if prior_rows is None else prior_rows[k], q) for k, q in groups.items()])
    return out


@pytest.mark.parametrize("alphabet_name", ["dna", "prot"])
@pytest.mark.parametrize("no_ends", [False, True])
def test_public_call_with_vanilla_models(alphabet_name, no_ends):
    lag, queries, seqs, reverse = SEQ_CASES[alphabet_name]
    assert any(len(s) == lag for s in queries)
    host = get_var_probs.make_sequence_counter(seqs, lag, reverse=reverse, no_end=no_ends, alphabet_name=alphabet_name)
    dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=reverse, no_end=no_ends, alphabet_name=alphabet_name)
    assert dev.no_end == no_ends
    strings = queries if no_ends else ["[" * lag + s + "]" for s in queries]
    kmers = get_var_probs._get_all_kmers_seqs(strings, lag)
    counts = host(kmers)
    assert (counts.sum(1) == 0).any()                                      # a k-mer the counter never saw
    kw = dict(vans=VANS, get_marg=True, lag=lag, alphabet_name=alphabet_name, no_ends=no_ends, counter=dev)
    got = get_var_probs.get_bear_probs_seqs(None, queries, 0, marg_on_device=True, **kw)
    default = get_var_probs.get_bear_probs_seqs(None, queries, 0, **kw)
    assert got.shape == default.shape == (len(queries), 3) and isinstance(got, np.ndarray) and got.dtype == np.float64
    W = len(core.alphabets_en[alphabet_name])
    want, mass = _closed_form(_string_groups(strings, lag, alphabet_name, dict(zip(kmers.tolist(), counts)), None), [], VANS, W)
    _check(got, want, mass, RTOL, f"public {alphabet_name} no_ends={no_ends}")
    _check(got, default, mass, 2 * RTOL, f"public {alphabet_name} no_ends={no_ends} against the default path")
    assert np.abs(default).max() > 1 and (mass.sum(1) == 0).any() == no_ends      # without pads a query of lag letters has no transition
    assert get_var_probs.get_bear_probs_seqs(None, [], 0, marg_on_device=True, **kw).shape == (0, 3)


def test_public_call_with_a_trained_folder(tmp_path):
    import configparser
    from bear_amd.models import train_bear_net
    lag = 4
    (tmp_path / "in").mkdir()
    table = _prot_table_600(tmp_path / "in", lag, seed=3)
    config = configparser.ConfigParser()
    config.read(os.path.join(ROOT, "bear_amd", "models", "config_files", "bear_test.cfg"))
    out = tmp_path / "out"
    config["general"]["out_folder"] = str(out) + "*"
    config["data"].update({"files_path": str(tmp_path / "in"), "start_token": "protk", "alphabet": "prot", "num_ds": "2",
                           "reference_column": "1"})
    config["hyperp"]["lag"] = str(lag)
    config["train"].update({"batch_size": "150", "epochs": "2", "train_ar": "False"})
    config["model"]["ar_func_name"] = "linear"
    exit_code, _, _ = train_bear_net.main(config)
    assert exit_code == 1
    _, alphabet, h, ar_func, data = get_var_probs.load_bear(str(out))
    assert alphabet == "prot" and data.num_rows == 600
    dev = get_var_probs.DeviceCounter.from_dataset(data, 0)
    seqs = [PROT_WT, "KKKKKKKKKKAKKKKKKKKKK", "MKTA", "WWWWWWCW", PROT_WT[::-1]]
    strings = ["[" * lag + s + "]" for s in seqs]
    kmers = get_var_probs._get_all_kmers_seqs(strings, lag)
    count_rows = {k: table.get(k, np.zeros(21)) for k in kmers.tolist()}
    assert sum(k in table for k in kmers.tolist()) > 10 and any(k not in table for k in kmers.tolist())
    prior = ar_func(torch.from_numpy(core.encode_kmers(kmers.tolist(), "prot")).to("cuda")).to(torch.float64).cpu().numpy()
    groups = _string_groups(strings, lag, "prot", count_rows, dict(zip(kmers.tolist(), prior)))
    for hs in (None, np.array([0.05, 3.0])):
        kw = dict(counter=dev, get_marg=True) if hs is None else dict(counter=dev, get_marg=True, h=hs)
        got = get_var_probs.get_bear_probs_seqs(str(out), seqs, 0, marg_on_device=True, **kw)
        default = get_var_probs.get_bear_probs_seqs(str(out), seqs, 0, **kw)
        n_h = 1 if hs is None else 2
        assert got.shape == default.shape == (len(seqs), n_h + 3)
        want, mass = _closed_form(groups, [h] if hs is None else hs, [0.1, 1.0, 10.0], 21)
        _check(got, want, mass, RTOL, f"trained folder, {n_h} h")
        _check(got, default, mass, 2 * RTOL, f"trained folder, {n_h} h, against the default path")
        assert np.abs(default).max() > 1


def test_refusals_before_any_launch(monkeypatch):
    dna = get_var_probs.DeviceCounter.from_sequences(SEQ_CASES["dna"][2], 3, alphabet_name="dna")

    def no_launch(*args):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(kernels, "_launch", no_launch)
    kw = dict(vans=VANS, lag=3, alphabet_name="dna", counter=dna, get_marg=True, marg_on_device=True)
    with pytest.raises(ValueError, match="'x'"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGT", "ACxGT"], 0, **kw)
    with pytest.raises(ValueError, match=r"'\]'"):
        get_var_probs.get_bear_probs_seqs(None, ["AC]GT"], 0, **kw)
    with pytest.raises(ValueError, match="lag"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, **dict(kw, lag=4))
    with pytest.raises(ValueError, match="'prot'"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, **dict(kw, alphabet_name="prot"))
