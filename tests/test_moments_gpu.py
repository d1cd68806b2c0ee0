"""GPU tests of the exact posterior mean and variance of scores on the device (kernels_moments.h, kernels.score_moments,
``moments=True`` of get_bear_probs / get_bear_probs_seqs): the kernel against the closed form evaluated with mpmath at 50 digits,
without and with signed weights; a segment's bits wherever it stands and in the deterministic library; the entry's edges and
refusals; the public calls against the closed form written out from the strings' own k-mers; and the sampled path's own mean and
variance at 4096 draws as a guard on the formula and the sign convention.

The closed form: with ``p ~ Dirichlet(a)`` the row of a k-mer under a model, ``A = sum_b a_b``, ``m_b`` the signed number of times a
score takes the transition (k-mer, b) and ``M = sum_b m_b``, the k-mer adds ``sum_b m_b psi(a_b) - M psi(A)`` to the mean and
``sum_b m_b^2 psi1(a_b) - M^2 psi1(A)`` to the variance; the k-mers are independent.

The bound everywhere (the figure and the L1-mass definition of tests/test_marg_gpu.py): ``|got - want| <= 1e-11 * mass`` per segment,
model and moment, ``mass`` the sum of ``|m psi(a)| + |M psi(A)|``, respectively ``m^2 psi1(a) + M^2 psi1(A)``.  A segment of mass 0 is
exactly 0; every other segment of the kernel case has a mass of at least 1e-3 (asserted on the mpmath side), so psi's root cannot
hide in the bound.  The largest ratio observed on an MI355X is recorded in DESIGN.md 4.7 (printed here per case)."""
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
from test_marg_gpu import HS, K, LENS, MODELS, RTOL, _dev, _kernel_case
from test_score_gpu import PROT_WT, VANS, _prot_table_600

pytestmark = pytest.mark.gpu

MIN_MASS = 1e-3
CANCEL, M_ZERO = len(LENS), len(LENS) + 1          # the two segments behind those of tests/test_marg_gpu.py


# ------------------------------------------------------------------------------------------- the closed form
def _row_values(c, f, hs, vans, W):
    """Per model ``(psi(a_j) [W], psi1(a_j) [W], psi(A), psi1(A))`` of one k-mer at 50 digits: ``a_j = f_j / h + c_j`` (BEAR) or
    ``van + c_j``."""
    out = []
    with mpmath.workdps(50):
        mpf = mpmath.mpf
        for m in range(len(hs) + len(vans)):
            if m < len(hs):
                a = [mpf(float(f[j])) / mpf(float(hs[m])) + int(c[j]) for j in range(W)]
            else:
                a = [mpf(float(vans[m - len(hs)])) + int(c[j]) for j in range(W)]
            A = mpmath.fsum(a)
            out.append(([mpmath.digamma(x) for x in a], [mpmath.polygamma(1, x) for x in a], mpmath.digamma(A), mpmath.polygamma(1, A)))
    return out


def _closed_form(groups_of_segments, n_models):
    """(want, mass) float64 [n_seg, n_models, 2]: per segment a list of groups ``(values, {letter: m})``, ``values`` the
    ``_row_values`` of the k-mer and ``m`` the signed multiplicity of its cell."""
    want, mass = np.zeros((len(groups_of_segments), n_models, 2)), np.zeros((len(groups_of_segments), n_models, 2))
    with mpmath.workdps(50):
        for s, groups in enumerate(groups_of_segments):
            for k in range(n_models):
                mean, var, l1_mean, l1_var = mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0)
                for values, q in groups:
                    psi, psi1, psi_A, psi1_A = values[k]
                    M = sum(q.values())
                    mean += mpmath.fsum(m * psi[j] for j, m in q.items()) - M * psi_A
                    var += mpmath.fsum(m * m * psi1[j] for j, m in q.items()) - M * M * psi1_A
                    l1_mean += mpmath.fsum(abs(m * psi[j]) for j, m in q.items()) + abs(M * psi_A)
                    l1_var += mpmath.fsum(m * m * psi1[j] for j, m in q.items()) + M * M * psi1_A
                want[s, k] = float(mean), float(var)
                mass[s, k] = float(l1_mean), float(l1_var)
    return want, mass


def _check(got, want, mass, what, rtol=RTOL):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = (err / np.where(mass > 0, mass, 1.0)).reshape(-1, 2).max(0)
    print(f"moments {what}: largest |got - want| / mass = {ratio[0]:.3e} (mean), {ratio[1]:.3e} (variance) (bound {rtol:.0e})")
    assert np.all(err <= rtol * mass), (what, ratio.tolist())
    assert not got[mass == 0].any()                        # nothing to sum: exactly 0


# ------------------------------------------------------------------------------------------- the kernel
def _moments_case(W):
    """The segments, count and prior rows of tests/test_marg_gpu.py, two more segments, and weights of +1 / -1 for every position:
    CANCEL, 400 positions followed by themselves with the opposite weights (every cell's m is 0); M_ZERO, row 8 with m = +2 and -2
    in two cells (M = 0, m != 0), row 11 with M = 1 and row 12 with m = 0 in its one cell."""
    segments, train, prior = _kernel_case(W)
    rng = np.random.default_rng(300 + W)
    rows, letters = rng.integers(0, K, 400), rng.integers(0, W, 400)
    sign = rng.choice(np.array([-1, 1], dtype=np.int8), 400)
    segments = list(segments) + [(np.r_[rows, rows].astype(np.int32), np.r_[letters, letters].astype(np.uint8)),
                                 (np.array([8, 11, 8, 12, 8, 8, 12], dtype=np.int32), np.array([1, 0, 1, 3, W - 1, W - 1, 3], dtype=np.uint8))]
    weights = [rng.choice(np.array([-1, 1], dtype=np.int8), len(r)) for r, _ in segments]
    weights[CANCEL] = np.r_[sign, -sign]
    weights[M_ZERO] = np.array([1, 1, 1, 1, -1, -1, -1], dtype=np.int8)
    return segments, weights, train, prior


def _score(segments, weights, train, prior, H, V, W):
    rows = np.concatenate([r for r, _ in segments] + [np.zeros(0, np.int32)])
    letters = np.concatenate([b for _, b in segments] + [np.zeros(0, np.uint8)])
    seg = np.concatenate([[0], np.cumsum([len(r) for r, _ in segments])]).astype(np.int64)
    w = None if weights is None else _dev(np.concatenate(list(weights) + [np.zeros(0, np.int8)]))
    got = kernels.score_moments(_dev(rows), _dev(letters), _dev(seg), _dev(train.view(np.int32)), _dev(prior) if H else None,
                                HS[:H] if H else None, VANS[:V] if V else None, weights=w)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (len(segments), H + V, 2)
    return got.cpu().numpy()


def _signed_counts(rows, letters, weights, W):
    groups = {}
    for r, b, w in zip(rows.tolist(), letters.tolist(), weights.tolist()):
        if r >= 0 and b < W:
            groups.setdefault(r, Counter())[b] += w
    return groups


@pytest.fixture(scope="module", params=[5, 21])
def kernel_case(request):
    """The case at one width and its closed form under all 3 + 3 models, without and with the weights, computed once."""
    W = request.param
    segments, weights, train, prior = _moments_case(W)
    values = [_row_values(train[r], prior[r], HS, VANS, W) for r in range(K)]
    refs = {}
    for weighted in (False, True):
        groups_of_segments = []
        for (rows, letters), w in zip(segments, weights):
            groups = _signed_counts(rows, letters, w if weighted else np.ones(len(rows), np.int8), W)
            groups_of_segments.append([(values[r], q) for r, q in groups.items()])
        refs[weighted] = _closed_form(groups_of_segments, len(HS) + len(VANS))
        if weighted:
            assert all(m == 0 for _, q in groups_of_segments[CANCEL] for m in q.values()) and len(groups_of_segments[CANCEL]) > 30
            assert sorted(tuple(sorted(q.items())) for _, q in groups_of_segments[M_ZERO]) == [((0, 1),), ((1, 2), (W - 1, -2)), ((3, 0),)]
        else:
            assert len(groups_of_segments[5]) == K and groups_of_segments[4][0][1] == {2: 3000}
        mass = refs[weighted][1]
        assert not mass[[i for i, n in enumerate(LENS) if n == 0]].any()
        assert (mass[CANCEL] == 0).all() == weighted
        live = [i for i, n in enumerate(LENS) if n > 0] + [M_ZERO] + ([] if weighted else [CANCEL])
        assert mass[live].min() >= MIN_MASS, (W, weighted, mass[live].min(1))
    return W, segments, weights, train, prior, refs


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("H,V", sorted(MODELS))
def test_kernel_against_the_closed_form(kernel_case, H, V, weighted):
    W, segments, weights, train, prior, refs = kernel_case
    want, mass = refs[weighted]
    got = _score(segments, weights if weighted else None, train, prior, H, V, W)
    cols = MODELS[(H, V)]
    _check(got, want[:, cols], mass[:, cols], f"kernel W={W} H={H} V={V} weighted={weighted}")
    assert all(not got[i].any() for i, n in enumerate(LENS) if n == 0)
    if weighted:
        assert np.array_equal(got[CANCEL].view(np.uint64), np.zeros_like(got[CANCEL]).view(np.uint64))      # exactly +0.0 and +0.0
    else:
        assert (got[5, :, 1] > 0).all() and np.abs(got[5, :, 0]).min() > 100
        ones = [np.ones(len(r), np.int8) for r, _ in segments]                                            # all +1: the same bits
        assert np.array_equal(got, _score(segments, ones, train, prior, H, V, W))
    assert np.array_equal(got, _score(segments, weights if weighted else None, train, prior, H, V, W))    # the same call twice: equal bits


@pytest.mark.parametrize("which", [6, 2, 5])
def test_a_segment_scores_the_same_wherever_it_stands(kernel_case, which):
    W, segments, weights, train, prior, _ = kernel_case

    def score(order):
        return _score([segments[i] for i in order], [weights[i] for i in order], train, prior, 3, 3, W)
    everything = list(range(len(segments)))
    whole = score(everything)
    alone = score([which])
    between = score([4, 1, which, 6, 2])                   # at offset 3001
    backwards = score(everything[::-1])
    assert np.abs(alone[0]).min() > 0
    for row in (whole[which], between[2], backwards[len(segments) - 1 - which]):
        assert row.tobytes() == alone[0].tobytes()
    assert np.array_equal(backwards[::-1], whole)


_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from bear_amd import _lib
import test_moments_gpu as t
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
segments, weights, train, prior = t._moments_case(21)
np.save(sys.argv[2], t._score(segments, weights, train, prior, 3, 3, 21))
"""


def test_deterministic_library_returns_the_same_bytes(tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    segments, weights, train, prior = _moments_case(21)
    here = _score(segments, weights, train, prior, 3, 3, 21)
    script = tmp_path / "det_moments.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npy")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    there = np.load(tmp_path / "det.npy")
    assert there.shape == here.shape and there.tobytes() == here.tobytes()


def test_edges_and_refusals(monkeypatch):
    train = torch.zeros((3, 5), dtype=torch.int32, device="cuda")
    none = torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.uint8, device="cuda")
    seg = torch.zeros(5, dtype=torch.int64, device="cuda")
    out = kernels.score_moments(*none, seg, train, None, None, VANS)
    assert out.shape == (4, 3, 2) and not out.any()
    assert kernels.score_moments(*none, seg[:1], train, None, None, VANS).shape == (0, 3, 2)             # n_seg = 0
    # positions, and no transition anywhere: a negative row, a row beyond the table, the skip letter, a letter beyond the width
    rows = torch.tensor([-1, 3, 0, 1], dtype=torch.int32, device="cuda")
    letters = torch.tensor([0, 0, kernels.SCORE_SKIP, 5], dtype=torch.uint8, device="cuda")
    seg4 = torch.tensor([0, 1, 4], dtype=torch.int64, device="cuda")
    for w in (None, torch.tensor([1, -1, 1, -1], dtype=torch.int8, device="cuda")):
        out = kernels.score_moments(rows, letters, seg4, train, None, None, VANS, weights=w)
        assert out.shape == (2, 3, 2) and np.array_equal(out.cpu().numpy().view(np.uint64), np.zeros((2, 3, 2), np.uint64))
    with pytest.raises(ValueError):
        kernels.score_moments(*none, seg, train, None, [1.0], VANS)                   # a BEAR model without prior rows
    with pytest.raises(ValueError):
        kernels.score_moments(*none, seg, train, None, None, [1.0, 0.0])              # a vanilla pseudo-count of 0
    prior = torch.ones((3, 5), dtype=torch.float64, device="cuda")
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            kernels.score_moments(*none, seg, train, prior, [1.0, bad], VANS)         # an h <= 0
    with pytest.raises(ValueError, match="1..16"):
        kernels.score_moments(*none, seg, train, None, None, np.ones(17))             # 17 models
    assert kernels.score_moments(*none, seg, train, None, None, np.ones(16)).shape == (4, 16, 2)
    with pytest.raises(ValueError, match="weights"):
        kernels.score_moments(rows, letters, seg4, train, None, None, VANS, weights=torch.tensor([1, 0, 1, -1], dtype=torch.int8, device="cuda"))
    with pytest.raises(ValueError, match="weights"):
        kernels.score_moments(rows, letters, seg4, train, None, None, VANS, weights=torch.ones(3, dtype=torch.int8, device="cuda"))
    monkeypatch.setattr(kernels, "_check_seg", lambda seg, device: 2 ** 53)           # (segments x 4 rows x 256 letters = 2^63)
    with pytest.raises(ValueError, match="63 bits"):
        kernels.score_moments(*none, seg, train, None, None, VANS)


# ------------------------------------------------------------------------------------------- the public calls
ALPHABETS = {"dna": "ACGT", "prot": "ACDEFGHIKLMNPQRSTVWY"}
PUBLIC = {"dna": (3, True), "prot": (2, False)}            # lag, reverse


def _random_sequences(alphabet_name, seed, n=200):
    """~200 sequences of 8 to 60 letters over the first 4 (dna) or 12 (prot) letters, so that the queries meet k-mers seen often,
    k-mers seen once and -- through the letters left out -- k-mers never seen."""
    rng = np.random.default_rng(seed)
    letters = np.array(list(ALPHABETS[alphabet_name][:12]))
    return ["".join(rng.choice(letters, int(rng.integers(8, 61)))) for _ in range(n)]


def _queries(alphabet_name, lag, seqs, seed):
    rng = np.random.default_rng(seed)
    letters = np.array(list(ALPHABETS[alphabet_name]))
    return [seqs[0], seqs[1][:lag], seqs[2][3:20] * 3, "".join(rng.choice(letters, 50)), letters[-1] * (lag + 4), seqs[3][::-1]]


def _variants(wt, alphabet_name, n_sub, seed):
    """Substitutions (the first and the last residue among them), one insertion, one deletion and a variant equal to the wild type."""
    rng = np.random.default_rng(seed)
    letters = ALPHABETS[alphabet_name]
    pos = [0, len(wt) - 1] + rng.integers(0, len(wt), n_sub - 2).tolist()
    subs = [f"{wt[p]}{p}{letters[(letters.index(wt[p]) + 1 + int(rng.integers(0, len(letters) - 1))) % len(letters)]}" for p in pos]
    return subs + [f"{wt[4]}4{wt[4]}{letters[1]}{letters[2]}", f"{wt[6:9]}6{wt[6]}", f"{wt[5]}5{wt[5]}"]


def _signed_strings(strings_and_signs, lag, alphabet_name):
    """{k-mer: {letter index: m}} of strings that count +1 or -1: every k+1-mer of every string, inside that string alone."""
    letter = {str(b): j for j, b in enumerate(core.alphabets_en[alphabet_name])}
    groups = {}
    for s, sign in strings_and_signs:
        for p in range(lag, len(s)):
            groups.setdefault(s[p - lag:p], Counter())[letter[s[p]]] += sign
    return groups


def _public_reference(signed_groups, count_rows, prior_rows, hs, vans, W):
    """``_closed_form`` of segments given as ``_signed_strings``; ``count_rows`` / ``prior_rows``: {k-mer: row} (prior None: vanilla)."""
    values = {}
    for groups in signed_groups:
        for k in groups:
            if k not in values:
                values[k] = _row_values(count_rows[k], None if prior_rows is None else prior_rows[k], hs, vans, W)
    return _closed_form([[(values[k], q) for k, q in groups.items()] for groups in signed_groups], len(hs) + len(vans))


def _variant_groups(wt, vars_, lag, alphabet_name):
    padded = "[" * lag + wt + "]"
    windows = get_var_probs._variant_windows([get_var_probs.parse_var(v) for v in vars_], padded, lag)
    return [_signed_strings([(windows[2 * i], 1), (windows[2 * i + 1], -1)], lag, alphabet_name) for i in range(len(vars_))]


def _rows_of(groups_list, counter, rows_of_kmers=None):
    """{k-mer: count row} (the counter called with the strings) and {k-mer: prior row} of every k-mer of the groups."""
    kmers = sorted({k for groups in groups_list for k in groups})
    counts = dict(zip(kmers, counter(np.array(kmers))))
    return kmers, counts, (None if rows_of_kmers is None else dict(zip(kmers, rows_of_kmers(kmers))))


def _check_variants(got, wt, vars_, lag, alphabet_name, counter, hs, vans, what, rows_of_kmers=None):
    groups = _variant_groups(wt, vars_, lag, alphabet_name)
    _, counts, priors = _rows_of(groups, counter, rows_of_kmers)
    W = len(core.alphabets_en[alphabet_name])
    want, mass = _public_reference(groups, counts, priors, hs, vans, W)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (len(vars_), len(hs) + len(vans), 2)
    _check(got, want, mass, what)
    assert (got[..., 1] >= 0).all() and not got[-1].any() and not mass[-1].any()      # the variant equal to the wild type: exactly 0, 0
    assert (mass[:-1] > 0).all() and np.abs(got[:-1, :, 0]).max() > 0.1
    return want


def _check_sequences(got, strings, lag, alphabet_name, counter, hs, vans, what, rows_of_kmers=None):
    groups = [_signed_strings([(s, 1)], lag, alphabet_name) for s in strings]
    _, counts, priors = _rows_of(groups, counter, rows_of_kmers)
    W = len(core.alphabets_en[alphabet_name])
    want, mass = _public_reference(groups, counts, priors, hs, vans, W)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (len(strings), len(hs) + len(vans), 2)
    _check(got, want, mass, what)
    assert (got[..., 1] >= 0).all() and np.abs(got[..., 0]).max() > 1
    return mass


@pytest.mark.parametrize("alphabet_name", ["dna", "prot"])
@pytest.mark.parametrize("no_ends", [False, True])
def test_public_sequences_with_vanilla_models(alphabet_name, no_ends):
    lag, reverse = PUBLIC[alphabet_name]
    seqs = _random_sequences(alphabet_name, 1)
    dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=reverse, no_end=no_ends, alphabet_name=alphabet_name)
    queries = _queries(alphabet_name, lag, seqs, 2)
    strings = queries if no_ends else ["[" * lag + s + "]" for s in queries]
    kw = dict(vans=VANS, lag=lag, alphabet_name=alphabet_name, no_ends=no_ends, counter=dev, moments=True)
    got = get_var_probs.get_bear_probs_seqs(None, queries, 0, **kw)
    mass = _check_sequences(got, strings, lag, alphabet_name, dev, [], VANS, f"sequences {alphabet_name} no_ends={no_ends}")
    assert (mass.sum((1, 2)) == 0).any() == no_ends       # without pads the query of lag letters has no transition
    # mc_samples and seed play no part, nor do the other queries of the call
    again = get_var_probs.get_bear_probs_seqs(None, queries[::-1], 0, mc_samples=3, seed=77, **kw)
    assert np.array_equal(again[::-1], got)
    assert get_var_probs.get_bear_probs_seqs(None, [], 0, **kw).shape == (0, 3, 2)


@pytest.mark.parametrize("alphabet_name", ["dna", "prot"])
def test_public_variants_with_vanilla_models(alphabet_name):
    lag, reverse = PUBLIC[alphabet_name]
    seqs = _random_sequences(alphabet_name, 3)
    dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=reverse, alphabet_name=alphabet_name)
    wt = seqs[0][:30] + ALPHABETS[alphabet_name][-1] + seqs[5][:9]
    vars_ = _variants(wt, alphabet_name, 24, 4)
    kw = dict(vans=VANS, lag=lag, alphabet_name=alphabet_name, counter=dev, moments=True)
    got = get_var_probs.get_bear_probs(None, wt, vars_, 0, **kw)
    _check_variants(got, wt, vars_, lag, alphabet_name, dev, [], VANS, f"variants {alphabet_name}")
    again = get_var_probs.get_bear_probs(None, wt, vars_[::-1], 0, mc_samples=3, seed=77, **kw)
    assert np.array_equal(again[::-1], got)
    assert get_var_probs.get_bear_probs(None, wt, [], 0, **kw).shape == (0, 3, 2)


def test_public_calls_with_a_trained_folder(tmp_path):
    """The folder of tests/test_marg_gpu.py::test_public_call_with_a_trained_folder."""
    import configparser
    from bear_amd.models import train_bear_net
    lag = 4
    (tmp_path / "in").mkdir()
    _prot_table_600(tmp_path / "in", lag, seed=3)
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

    def rows_of_kmers(kmers):
        return ar_func(torch.from_numpy(core.encode_kmers(kmers, "prot")).to("cuda")).to(torch.float64).cpu().numpy()
    seqs = [PROT_WT, "KKKKKKKKKKAKKKKKKKKKK", "MKTA", "WWWWWWCW", PROT_WT[::-1]]
    strings = ["[" * lag + s + "]" for s in seqs]
    vars_ = _variants(PROT_WT, "prot", 10, 5)
    vans = [0.1, 1.0, 10.0]
    for hs in (None, np.array([0.05, 3.0])):
        kw = dict(counter=dev, moments=True) if hs is None else dict(counter=dev, moments=True, h=hs)
        models = [h] if hs is None else hs
        got = get_var_probs.get_bear_probs_seqs(str(out), seqs, 0, **kw)
        _check_sequences(got, strings, lag, "prot", dev, models, vans, f"trained folder, sequences, {len(models)} h", rows_of_kmers)
        got = get_var_probs.get_bear_probs(str(out), PROT_WT, vars_, 0, **kw)
        _check_variants(got, PROT_WT, vars_, lag, "prot", dev, models, vans, f"trained folder, variants, {len(models)} h", rows_of_kmers)


def test_public_calls_with_a_reference_model():
    lag, name = 3, "dna"
    train, ref = _random_sequences(name, 6), _random_sequences(name, 7, n=60)
    counter = get_var_probs.DeviceCounter.from_sequences(train, lag, reverse=False, alphabet_name=name)
    ref_counter = get_var_probs.DeviceCounter.from_sequences(ref, lag, reverse=False, alphabet_name=name)
    model = get_var_probs.RefModel(lag, name, 0.3, 0.2, 0.3)
    former = get_var_probs._RefRows(model, ref_counter)

    def rows_of_kmers(kmers):                              # the rows the scoring paths take, of the k-mers as strings
        raw = np.frombuffer("".join(kmers).encode("ascii"), dtype=np.uint8)
        keys = counter._keys_of_codes(torch.from_numpy(counter._lut[raw].reshape(len(kmers), lag)).to("cuda"))
        return former.rows(counter, keys).cpu().numpy()
    kw = dict(vans=VANS, counter=counter, ref_model=model, ref_counter=ref_counter, moments=True)
    queries = _queries(name, lag, train, 8)
    wt = train[0][:30] + "T" + train[5][:9]
    vars_ = _variants(wt, name, 12, 9)
    for hs in (None, [0.05, 4.0]):
        models = [model.h] if hs is None else hs
        got = get_var_probs.get_bear_probs_seqs(None, queries, 0, h=hs, **kw)
        _check_sequences(got, ["[" * lag + s + "]" for s in queries], lag, name, counter, models, VANS,
                         f"reference model, sequences, {len(models)} h", rows_of_kmers)
        got = get_var_probs.get_bear_probs(None, wt, vars_, 0, h=hs, **kw)
        _check_variants(got, wt, vars_, lag, name, counter, models, VANS, f"reference model, variants, {len(models)} h", rows_of_kmers)


def test_refusals_before_any_launch(monkeypatch):
    dna = get_var_probs.DeviceCounter.from_sequences(_random_sequences("dna", 1, n=20), 3, alphabet_name="dna")

    def no_launch(*args):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(kernels, "_launch", no_launch)
    kw = dict(vans=VANS, lag=3, alphabet_name="dna", counter=dna, moments=True)
    with pytest.raises(ValueError, match="'x'"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGT", "ACxGT"], 0, **kw)
    with pytest.raises(ValueError, match="lag"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, **dict(kw, lag=4))
    with pytest.raises(ValueError, match="get_marg"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, get_marg=True, **kw)
    with pytest.raises(ValueError, match="get_map"):
        get_var_probs.get_bear_probs(None, "ACGTACGT", ["A0C"], 0, get_map=True, **kw)
    with pytest.raises(ValueError, match="DeviceCounter"):
        get_var_probs.get_bear_probs(None, "ACGTACGT", ["A0C"], 0, **dict(kw, counter=lambda kmers: None))


# ------------------------------------------------------------------------------------------- against the sampled path
def test_consistency_with_the_sampled_path():
    """A guard on the formula and the sign convention, not a precision claim: the same get_bear_probs call with 4096 samples and a
    fixed seed; the sample mean within 6 standard errors of the exact mean (at most 1e3 comparisons: a correct implementation
    fails with probability below 2e-6, and the seed is fixed), the sample variance within a factor 2 of the exact variance.
    Every concentration is at least 0.5 (vanilla models 0.5, 1, 10, no BEAR model), so that the central limit holds at 4096 draws."""
    lag, name, n_mc = 3, "dna", 4096
    seqs = _random_sequences(name, 10)
    dev = get_var_probs.DeviceCounter.from_sequences(seqs, lag, reverse=True, alphabet_name=name)
    wt = seqs[0][:40]
    vars_ = [f"{wt[p]}{p}{b}" for p in range(len(wt)) for b in "ACGT" if b != wt[p]] + _variants(wt, name, 2, 11)[2:]
    vans = (0.5, 1.0, 10.0)
    kw = dict(vans=vans, lag=lag, alphabet_name=name, counter=dev)
    exact = get_var_probs.get_bear_probs(None, wt, vars_, 0, moments=True, **kw)
    sampled = get_var_probs.get_bear_probs(None, wt, vars_, 0, mc_samples=n_mc, seed=12345, **kw)
    assert sampled.shape == (len(vars_), 3, n_mc) and exact.shape == (len(vars_), 3, 2) and exact.size // 2 <= 1000
    mean, var = exact[..., 0], exact[..., 1]
    mean_mc, var_mc = sampled.mean(-1), sampled.var(-1, ddof=1)
    z = np.abs(mean_mc - mean) / np.sqrt(np.where(var > 0, var, 1.0) / n_mc)
    ratio = var_mc[var > 0] / var[var > 0]
    print(f"moments against {n_mc} samples: largest |mean_mc - mean| / standard error = {z[var > 0].max():.2f} (bound 6), "
          f"var_mc / var in [{ratio.min():.3f}, {ratio.max():.3f}] (bounds 0.5, 2)")
    assert np.all(np.abs(mean_mc - mean) <= 6 * np.sqrt(var / n_mc))
    assert (var > 0).sum() >= 3 * (len(vars_) - 1) and np.all((0.5 <= ratio) & (ratio <= 2))
    assert not exact[-1].any() and not sampled[-1].any()                               # the variant equal to the wild type
