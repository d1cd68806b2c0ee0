"""CPU tests of the segmentation (kernels_segment.h, bear_score_emit_groups_f64, bear_hmm_groups_f64, bear_amd.classify.segment): the
two entries in the header, the binding and both libraries, their refusals before any device call, the refusals of the Python
layers without a device, and the oracles of tests/segment_util.py against brute force, against each other and on the
statistical case."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import segment_util as sg
from util import abi_header

EMIT, HMM = "bear_score_emit_groups_f64", "bear_hmm_groups_f64"
NEG = float("-inf")


def test_entries_declared_with_the_stream_not_last_and_exported_by_both_libraries():
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    want = {EMIT: [vp, vp, u64, i, vp, i, vp, u64, vp, i, vp, i, vp, vp], HMM: [vp, u64, vp, u64, i, vp, vp, vp, vp, vp, vp, vp]}
    header = open(_lib.HEADER_PATH).read()
    det = ctypes.CDLL(_lib.LIB_PATH.replace("libbear_hip.so", "libbear_hip_det.so"))
    assert version == _lib.ABI_VERSION == 12                 # entries are added without a new version
    for name, stream_at, last in ((EMIT, 12, ["double *emit"]), (HMM, 7, ["uint8_t *path", "double *log_post"])):
        assert name in _lib.SYMBOLS and sigs[name] == (i, want[name]) and _lib._SIGNATURES[name] == (i, want[name])
        decl = re.search(r"^int %s\(([^)]*)\);" % name, header, flags=re.M | re.S)
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        assert params[stream_at] == "void *stream" and params[-len(last):] == last and len(params) == len(want[name])
        fn = getattr(_lib.lib(), name)
        assert fn.restype is i and list(fn.argtypes) == want[name]
        assert hasattr(det, name)
    assert "#define BEAR_HMM_MAX_STATES %d" % kernels.HMM_MAX_STATES in header and kernels.HMM_MAX_STATES == 16
    assert "#define BEAR_HMM_CHUNK %d" % kernels.HMM_CHUNK in header
    assert list(inspect.signature(kernels.emit_groups).parameters) == ["rows", "letters", "train", "prior", "h", "vans"]
    assert list(inspect.signature(kernels.hmm_groups).parameters) == ["emit", "seg", "log_trans", "log_start", "want_post"]


def _emit(width=5, prior=None, K=10, G=3, h=(), van=(0.1, 1.0), n_h=None, n_van=None, rows=None, letters=None, n_t=0, train=None, emit=None):
    """The emission entry with host vectors h / van and the given (fake) device addresses: every case returns before a device call."""
    from bear_amd import _lib
    h, van = np.asarray(h, dtype=np.float64), np.asarray(van, dtype=np.float64)
    return _lib.lib().bear_score_emit_groups_f64(rows, letters, n_t, width, train, G, prior, K, h.ctypes.data if h.size else None,
                                                 h.size if n_h is None else n_h, van.ctypes.data if van.size else None,
                                                 van.size if n_van is None else n_van, None, emit)


def test_emission_arguments_are_checked_before_any_device_call():
    from bear_amd import kernels
    assert _emit() == 0                                               # n_t == 0: nothing to launch
    assert _emit(width=21, h=(0.05, 3.0), prior=0x1000, G=kernels.GROUPS_MAX) == 0
    for G in (0, -1, kernels.GROUPS_MAX + 1):
        assert _emit(G=G) == -1
    for width in (0, 4, 6, 20, 22):
        assert _emit(width=width) == -1
    assert _emit(h=(1.0,), prior=None) == -1
    for bad in (0.0, -1.0, float("nan")):
        assert _emit(van=(1.0, bad)) == -1
        assert _emit(h=(bad, 1.0), prior=0x1000) == -1
    assert _emit(van=()) == -1
    assert _emit(van=np.ones(kernels.MARG_MAX_MODELS)) == 0 and _emit(van=np.ones(kernels.MARG_MAX_MODELS + 1)) == -1
    assert _emit(n_h=-1) == -1 and _emit(n_van=-1) == -1
    assert _emit(K=2 ** 32 - 1) == -1 and _emit(K=2 ** 32 - 2) == 0
    assert _emit(h=(1.0,), prior=0x5004) == -1                        # a misaligned prior, with or without positions
    ok = dict(n_t=4, rows=0x1000, letters=0x1001, train=0x3000, emit=0x4000)
    for name in ("rows", "letters", "train", "emit"):
        assert _emit(**dict(ok, **{name: None})) == -1, name
    for name, address in (("rows", 0x1002), ("train", 0x3002), ("emit", 0x4004)):
        assert _emit(**dict(ok, **{name: address})) == -1, name
    assert _emit(**dict(ok, n_t=2 ** 61)) == -1                       # more values than a size holds


def _hmm(S=2, lt=None, ls=None, n_t=0, n_seg=0, emit=None, seg=None, ev=None, best=None, path=None, post=None, no_lt=False, no_ls=False):
    from bear_amd import _lib
    lt = np.ascontiguousarray(np.zeros((max(S, 1), max(S, 1))) if lt is None else lt, dtype=np.float64)
    ls = np.ascontiguousarray(np.zeros(max(S, 1)) if ls is None else ls, dtype=np.float64)
    return _lib.lib().bear_hmm_groups_f64(emit, n_t, seg, n_seg, S, None if no_lt else lt.ctypes.data, None if no_ls else ls.ctypes.data,
                                          None, ev, best, path, post)


def test_chain_arguments_are_checked_before_any_device_call():
    from bear_amd import kernels
    assert _hmm() == 0 and _hmm(S=1) == 0 and _hmm(S=kernels.HMM_MAX_STATES) == 0          # n_seg == 0: nothing to launch
    for S in (0, -1, kernels.HMM_MAX_STATES + 1):
        assert _hmm(S=S) == -1
    assert _hmm(no_lt=True) == -1 and _hmm(no_ls=True) == -1
    assert _hmm(lt=[[0.0, NEG], [NEG, -1.0]], ls=[NEG, 0.0]) == 0                           # -inf is allowed, rows need no norm
    for bad in (float("nan"), float("inf")):
        assert _hmm(lt=[[0.0, bad], [0.0, 0.0]]) == -1 and _hmm(ls=[0.0, bad]) == -1
    assert _hmm(lt=[[0.0, 0.0], [NEG, NEG]]) == -1 and _hmm(ls=[NEG, NEG]) == -1            # a row / a start without a finite entry
    assert _hmm(post=0x7004) == -1 and _hmm(post=0x7008) == 0                               # misaligned, with or without segments
    ok = dict(n_seg=1, n_t=4, emit=0x1000, seg=0x2000, ev=0x3000, best=0x4000, path=0x5001, post=0x7000)
    for name in ("emit", "seg", "ev", "best", "path"):
        assert _hmm(**dict(ok, **{name: None})) == -1, name
    for name, address in (("emit", 0x1004), ("seg", 0x2004), ("ev", 0x3004), ("best", 0x4004), ("post", 0x7004)):
        assert _hmm(**dict(ok, **{name: address})) == -1, name
    assert _hmm(**dict(ok, n_t=2 ** 61)) == -1


def _hollow_counter(G=3, alphabet="dna", lag=2):
    """A GroupCounter that holds no table: every refusal below comes before it is looked at."""
    import torch
    from bear_amd import classify
    counter = object.__new__(classify.GroupCounter)
    counter.counts = torch.zeros((0, G, 5 if alphabet == "dna" else 21), dtype=torch.int32)
    counter.lag, counter.alphabet_name, counter.reverse = lag, alphabet, False
    return counter


def test_python_refusals_need_no_device(monkeypatch):
    import torch
    from bear_amd import classify, get_var_probs, kernels, _lib

    def no_device(*args, **kwargs):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(kernels, "_launch", no_device)
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(get_var_probs, "_device", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    models = ["vans", "bear_path", "ar_func", "h", "no_ends"]
    assert list(inspect.signature(classify.position_log_probs).parameters) == ["counter", "seqs"] + models
    assert list(inspect.signature(classify.segment).parameters) == ["counter", "seqs", "switch", "log_trans", "log_start", "model",
                                                                    "posterior"] + models
    for fn in (classify.position_log_probs, classify.segment):
        assert all(p.kind is p.KEYWORD_ONLY for p in list(inspect.signature(fn).parameters.values())[2:])
    counter = _hollow_counter()

    def uniform(codes):
        raise AssertionError("the AR function was called")
    # the refusals of hypothesis._check_model, in both calls
    for kw in (dict(), dict(ar_func=uniform), dict(h=1.0), dict(bear_path="somewhere", ar_func=uniform, h=1.0), dict(vans=[1.0, 0.0]),
               dict(vans=[float("inf")]), dict(ar_func=uniform, h=[1.0, -2.0]), dict(vans=np.ones(17))):
        with pytest.raises(ValueError):
            classify.position_log_probs(counter, ["ACGT"], **kw)
        with pytest.raises(ValueError):
            classify.segment(counter, ["ACGT"], switch=0.01, **kw)
    for fn, kw in ((classify.position_log_probs, {}), (classify.segment, dict(switch=0.01))):
        with pytest.raises(ValueError, match="GroupCounter"):
            fn(object.__new__(get_var_probs.DeviceCounter), ["ACGT"], vans=[1.0], **kw)
    with pytest.raises(ValueError, match="17 groups"):
        classify.segment(_hollow_counter(G=17), ["ACGT"], vans=[1.0], switch=0.01)
    # the chain: exactly one of switch and log_trans; a switch in (0, 1), with a uniform start and another group to go to
    eye = np.log(np.full((3, 3), 0.01) + 0.97 * np.eye(3))
    for kw in (dict(), dict(switch=0.01, log_trans=eye), dict(switch=0.0), dict(switch=1.0), dict(switch=-0.1), dict(switch=float("nan")),
               dict(switch=0.01, log_start=np.zeros(3)), dict(log_trans=eye[:2]), dict(log_trans=eye, log_start=np.zeros(2)),
               dict(log_trans=np.where(np.eye(3) > 0, np.nan, eye)), dict(log_trans=np.where(np.eye(3) > 0, np.inf, eye)),
               dict(log_trans=np.where(np.arange(3)[:, None] == 1, NEG, eye)), dict(log_trans=eye, log_start=[NEG] * 3),
               dict(log_trans=eye, log_start=[0.0, float("nan"), 0.0])):
        with pytest.raises(ValueError):
            classify.segment(counter, ["ACGT"], vans=[1.0], **kw)
    with pytest.raises(ValueError, match="one group"):
        classify.segment(_hollow_counter(G=1), ["ACGT"], vans=[1.0], switch=0.01)
    for model in (-1, 2, 1.0, True):
        with pytest.raises(ValueError, match="model"):
            classify.segment(counter, ["ACGT"], vans=[1.0, 2.0], switch=0.01, model=model)
    with pytest.raises(ValueError, match="model"):
        classify.segment(counter, ["ACGT"], ar_func=uniform, h=[1.0], vans=[1.0], switch=0.01, model=2)
    # kernels.emit_groups, kernels.hmm_groups and kernels.check_chain: what is checked before the first launch
    with pytest.raises(ValueError, match="train"):
        kernels.emit_groups(None, None, torch.zeros((4, 3, 5), dtype=torch.int32), None, None, [1.0])
    with pytest.raises(ValueError, match="train"):
        kernels.emit_groups(None, None, torch.zeros((4, 5), dtype=torch.int32), None, None, [1.0])
    with pytest.raises(ValueError, match="emit"):
        kernels.hmm_groups(torch.zeros((4, 3), dtype=torch.float64), None, eye, np.zeros(3))
    lt, ls = kernels.check_chain(eye.tolist(), [0.0, NEG, NEG], 3)
    assert lt.dtype == ls.dtype == np.float64 and lt.flags.c_contiguous and lt.shape == (3, 3) and ls.shape == (3,)
    for S in (0, 17):
        with pytest.raises(ValueError, match="states"):
            kernels.check_chain(np.zeros((S, S)), np.zeros(S), S)


def test_runs_tile_the_transitions():
    from bear_amd import classify
    seg = classify.Segmentation("van(1)", np.array([0, 6, 6, 7]), np.array([0, 0, 2, 2, 2, 0, 1], dtype=np.uint8), None, None, None)
    assert seg.runs(0) == [(0, 2, 0), (2, 5, 2), (5, 6, 0)] and seg.runs(1) == [] and seg.runs(2) == [(0, 1, 1)]


# ------------------------------------------------------------------------------------------- the oracles
@pytest.mark.parametrize("S", [1, 2, 3])
def test_oracles_against_brute_force_over_all_paths(S):
    """Evidence, posterior, best and path of the 50-digit oracle and of its longdouble twin against the enumeration of all S^T
    paths, T <= 6, under every chain of ``sg.chains`` -- the left-to-right one has -inf transitions and a one-state start."""
    rng = np.random.default_rng(S)
    seen_inf = False
    for T in (1, 2, 3, 5, 6):
        for name, (lt, ls) in sg.chains(S).items():
            e = rng.normal(-2.0, 1.5, (T, S))
            brute = sg.brute_force(e, lt, ls)
            for solve in (sg.chain_oracle, sg.chain_twin):
                got = solve(e, lt, ls)
                for k in ("log_evidence", "log_best"):
                    assert abs(got[k] - brute[k]) <= 1e-14 * abs(brute[k]), (S, T, name, k)
                finite = np.isfinite(brute["log_post"])
                assert np.array_equal(got["log_post"][~finite], brute["log_post"][~finite])          # -inf exactly where it is
                assert np.abs(got["log_post"][finite] - brute["log_post"][finite]).max() <= 1e-13
                assert np.array_equal(got["path"], brute["path"])
                if len(brute["winners"]) == 1:            # a unique best path: the max-marginals' arg-max IS the Viterbi path
                    assert got["path"].tolist() == list(brute["winners"][0])
                assert np.abs(np.exp(got["log_post"]).sum(1) - 1.0).max() <= 1e-12
            seen_inf = seen_inf or bool(np.isneginf(brute["log_post"]).any())
    assert seen_inf == (S > 1)


def test_oracle_without_a_step_and_without_a_path():
    lt, ls = sg.chains(3)["dense"]
    for solve in (sg.chain_oracle, sg.chain_twin):
        none = solve(np.zeros((0, 3)), lt, ls)
        assert abs(none["log_evidence"] - np.log(np.exp(ls).sum())) <= 1e-14 and none["log_best"] == ls.max() and none["path"].size == 0
        # the chain must alternate from state 0, the second step's emission rules state 1 out: no path is left
        dead = solve(np.array([[0.0, NEG], [0.0, NEG], [0.0, 0.0]]), [[NEG, 0.0], [0.0, NEG]], [0.0, NEG])
        assert dead["log_evidence"] == NEG and dead["log_best"] == NEG and np.isnan(dead["log_post"]).all() and (dead["path"] == 255).all()


def test_every_chain_case_is_decided_by_the_oracle():
    """The seeds of ``sg.CHAIN_SEEDS`` were chosen here: in every case of tests/test_segment_gpu.py the oracle's best and second-best
    max-marginal lie more than 1e-6 apart at every step, so ``path`` is compared exactly and no position is left out."""
    from bear_amd import kernels
    for S in (1, 2, 3, 16):
        for name in sg.chains(S):
            emit, seg, lt, ls, want, mass = sg.chain_case(S, name, kernels.HMM_CHUNK)
            assert seg[-1] == emit.shape[0] and len(want) == len(sg.chain_lengths(S, kernels.HMM_CHUNK))
            assert min(float(w["gap"].min()) if w["gap"].size else np.inf for w in want) > sg.MIN_GAP, (S, name)
            assert all(np.isfinite(w["log_evidence"]) and np.isfinite(w["log_best"]) for w in want)
            if name == "left_to_right" and S > 1:
                assert any(np.isneginf(w["log_post"]).any() for w in want)
    # the twin on a case of the 50-digit oracle, beyond one chunk
    emit, seg, lt, ls, want, mass = sg.chain_case(3, "dense", kernels.HMM_CHUNK)
    a, b = seg[3], seg[4]
    twin = sg.chain_twin(emit[a:b], lt, ls)
    assert abs(twin["log_evidence"] - want[3]["log_evidence"]) <= 1e-14 * mass[3] and np.array_equal(twin["path"], want[3]["path"])
    assert np.abs(twin["log_post"] - want[3]["log_post"]).max() <= 1e-14 * mass[3]


def test_statistical_case_is_decided_by_the_oracle_alone():
    """40 chimeras of 600 letters per alphabet (``sg.stat_chimeras``), van(1), switch probability 0.005: the oracle's Viterbi labels
    against the truth -- dna lag 1 / 2 0.983 / 0.985, prot lag 1 / 2 0.995 / 0.993 -- and no position within 1e-6 of a tie (the
    smallest gap is 2e-3).  One label per sequence, which is all ``classify`` gives, cannot do better than the longer side."""
    for alphabet in ("dna", "prot"):
        seqs, truth = sg.stat_chimeras(alphabet)
        assert len(seqs) == sg.STAT_N and all(len(s) == sg.STAT_LEN and 0 < t.sum() < sg.STAT_LEN for s, t in zip(seqs, truth))
        longer_side = np.mean([max(t.mean(), 1 - t.mean()) for t in truth])
        for lag in (1, 2):
            paths, gap, accuracy = sg.stat_oracle(alphabet, lag)
            assert gap > sg.MIN_GAP and accuracy >= 0.9 and accuracy > longer_side, (alphabet, lag, gap, accuracy)
