"""GPU tests of the group classifier (kernels_groups.h, kernels.score_groups, bear_amd.classify): the kernel against the formula
evaluated with mpmath at 50 digits (tests/classify_util.py) at both widths, leave-one-out groups included; its bits against
``kernels.score_marg`` column by column, alone and inside a text, and from the deterministic library; what an underflow leaves; a
text beyond one grid's reach; the stream contract of include/bear_hip.h on a side stream (the entry's stream is not its last
parameter, so tests/test_stream_contract_gpu.py does not see it: same harness, here); the public calls, and a statistical case.

The bound: ``|got - want| <= 1e-11 * mass``, ``mass`` the L1 sum of the lgamma brackets behind a score -- the figure of
tests/test_marg_gpu.py for this item routine and these sums.  The largest ratio observed on an MI355X is printed per case and
recorded in DESIGN.md 4.7."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classify_util as cu
import stream_util as su
import two_sample_util as tu
from bear_amd import classify, get_var_probs, kernels
from classify_util import G, HS, K, LENS, OWN, RTOL, VANS
from conftest import ROOT

pytestmark = pytest.mark.gpu

MODELS = {(2, 3): [0, 1, 2, 3, 4], (0, 1): [2]}            # (BEAR, vanilla) models of a call -> columns of the oracle's 2 + 3


def _dev(a):
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _text(segments):
    rows = np.concatenate([r for r, _ in segments] + [np.zeros(0, np.int32)])
    letters = np.concatenate([b for _, b in segments] + [np.zeros(0, np.uint8)])
    seg = np.concatenate([[0], np.cumsum([len(r) for r, _ in segments])]).astype(np.int64)
    return _dev(rows), _dev(letters), _dev(seg)


def _groups(segments, train, prior, H, V, own=None):
    """(scores [n_seg, G, H + V], short_of [n_seg]) of ``kernels.score_groups`` as NumPy arrays."""
    own = None if own is None else _dev(np.asarray(own, dtype=np.int32))
    scores, short_of = kernels.score_groups(*_text(segments), _dev(train), _dev(prior) if H else None, HS[:H] if H else None,
                                            VANS[:V] if V else None, own=own)
    assert scores.is_cuda and scores.dtype == torch.float64 and scores.shape == (len(segments), train.shape[1], H + V)
    assert short_of.is_cuda and short_of.dtype == torch.uint8 and short_of.shape == (len(segments),)
    return scores.cpu().numpy(), short_of.cpu().numpy()


def _marg(segments, column, prior, H, V):
    return kernels.score_marg(*_text(segments), _dev(np.ascontiguousarray(column)), _dev(prior) if H else None, HS[:H] if H else None,
                              VANS[:V] if V else None).cpu().numpy()


def _check(got, want, mass, what, rtol=RTOL):
    err = np.abs(got - want)
    ratio = float((err / np.where(mass > 0, mass, 1.0)).max()) if got.size else 0.0
    print(f"classify {what}: largest |got - want| / mass = {ratio:.3e} (bound {rtol:.0e})")
    assert got.shape == want.shape and np.all(err <= rtol * mass), (what, ratio)
    assert not got[mass == 0].any()                        # nothing to sum: exactly 0


@pytest.fixture(scope="module", params=[5, 21])
def case(request):
    """The kernel case at one width and its oracle under 2 + 3 models with the own groups of OWN, computed once."""
    W = request.param
    segments, train, prior = cu.kernel_case(W)
    entries = [cu.segment_entries(s, train, prior, W) for s in segments]
    assert len(entries[5]) >= K - 2 and len(entries[2]) == 3 and entries[4][0][2] == {2: 3000} and 3000 > kernels.MARG_CHUNK > 41
    want, mass = cu.oracle(entries, HS, VANS, W, G, OWN)
    assert np.isfinite(want).all()
    return W, segments, train, prior, want, mass


@pytest.mark.parametrize("H,V", sorted(MODELS))
def test_kernel_against_the_oracle(case, H, V):
    W, segments, train, prior, want, mass = case
    got, short_of = _groups(segments, train, prior, H, V, OWN)
    cols = MODELS[(H, V)]
    _check(got, want[:, :, cols], mass[:, :, cols], f"kernel W={W} H={H} V={V}")
    assert not short_of.any()
    assert all(not got[i].any() for i, n in enumerate(LENS) if n == 0) and np.abs(got[5]).min() > 100
    again, _ = _groups(segments, train, prior, H, V, OWN)
    assert again.tobytes() == got.tobytes()                # the same call twice: equal bits


def test_without_own_every_group_has_the_bits_of_score_marg(case):
    W, segments, train, prior, _, _ = case
    for H, V in MODELS:
        got, short_of = _groups(segments, train, prior, H, V)
        assert not short_of.any()
        for g in range(G):
            assert np.ascontiguousarray(got[:, g]).tobytes() == _marg(segments, train[:, g], prior, H, V).tobytes(), (H, V, g)
    out_of_range, _ = _groups(segments, train, prior, 2, 3, [-1, 7, G, -5, 2 ** 31 - 1, -2 ** 31, 255, 256])
    assert out_of_range.tobytes() == _groups(segments, train, prior, 2, 3)[0].tobytes()     # a group that is none: as without own


def test_own_group_has_the_bits_of_score_marg_on_the_column_less_the_segment(case):
    W, segments, train, prior, _, _ = case
    got, _ = _groups(segments, train, prior, 2, 3, OWN)
    plain, _ = _groups(segments, train, prior, 2, 3)
    seen = 0
    for s, own in enumerate(OWN):
        others = [g for g in range(G) if g != own]
        assert np.ascontiguousarray(got[s, others]).tobytes() == np.ascontiguousarray(plain[s, others]).tobytes(), s
        if 0 <= own < G and LENS[s]:
            less = train[:, own] - cu.counts_of(segments[s], K, W)
            assert (less <= train[:, own]).all()           # the table held the segment: nothing wrapped
            assert got[s, own].tobytes() == _marg([segments[s]], less, prior, 2, 3)[0].tobytes(), s
            assert (got[s, own] != plain[s, own]).all()
            seen += 1
    assert seen == 3
    assert not (train[3, 0] - cu.counts_of(segments[1], K, W)[3]).any()      # segment 1: c_j == q_j for a whole row


@pytest.mark.parametrize("which", [1, 4, 5, 6])
def test_a_segment_scores_the_same_alone_as_inside_the_text(case, which):
    W, segments, train, prior, _, _ = case
    whole, _ = _groups(segments, train, prior, 2, 3, OWN)
    alone, short_of = _groups([segments[which]], train, prior, 2, 3, [OWN[which]])
    assert not short_of.any() and np.abs(alone).min() > 1
    assert alone[0].tobytes() == whole[which].tobytes()
    order = [4, 1, which, 6, 2]                             # at another offset, between other segments
    between, _ = _groups([segments[i] for i in order], train, prior, 2, 3, [OWN[i] for i in order])
    assert between[2].tobytes() == alone[0].tobytes()


_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from bear_amd import _lib
import classify_util as cu
import test_classify_gpu as t
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
segments, train, prior = cu.kernel_case(21)
scores, short_of = t._groups(segments, train, prior, 2, 3, cu.OWN)
np.savez(sys.argv[2], scores=scores, short_of=short_of)
"""


def test_deterministic_library_returns_the_same_bits(tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    segments, train, prior = cu.kernel_case(21)
    scores, short_of = _groups(segments, train, prior, 2, 3, OWN)
    script = tmp_path / "det_classify.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npz")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    there = np.load(tmp_path / "det.npz")
    assert there["scores"].shape == scores.shape and there["scores"].tobytes() == scores.tobytes()
    assert there["short_of"].tobytes() == short_of.tobytes()


def test_underflow_marks_the_segment_alone(case):
    """Segment 6 claims group 1, which lacks some of its transitions: short_of for that segment alone, its own-group scores NaN, and
    every other score of the call the bits of the call in which segment 6 has no own group (OWN: its 7 is none)."""
    W, segments, train, prior, _, _ = case
    assert (cu.counts_of(segments[6], K, W) > train[:, 1]).any()
    claimed = list(OWN)
    claimed[6] = 1
    base, _ = _groups(segments, train, prior, 2, 3, OWN)
    got, short_of = _groups(segments, train, prior, 2, 3, claimed)
    assert short_of.tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    assert np.isnan(got[6, 1]).all()
    keep = np.ones(got.shape, dtype=bool)
    keep[6, 1] = False
    assert np.isfinite(got[keep]).all() and got[keep].tobytes() == base[keep].tobytes()
    # a run that the own group holds too rarely while the k-mer's other letters are there: the run's own cell decides
    rows, letters = np.array([9, 9, 9, 9], dtype=np.int32), np.array([2, 2, 2, 0], dtype=np.uint8)
    few = train.copy()
    few[9, 0, 2], few[9, 0, 0] = 2, 5
    got, short_of = _groups([(rows, letters), segments[2]], few, prior, 2, 3, [0, -1])
    assert short_of.tolist() == [1, 0] and np.isnan(got[0, 0]).all() and np.isfinite(got[0, 1:]).all() and np.isfinite(got[1]).all()


def test_text_beyond_one_grid():
    """The host caps the terms kernel's grid at 2^20 blocks of 256 threads and the kernel strides: behind 2^28 positions without a
    transition (one segment, summed in chunks) the segments of the case have the bits they have alone.  (Width 5, one vanilla
    model: the stride depends on neither.)"""
    segments, train, prior = cu.kernel_case(5)
    pick = [1, 2, 4, 6]
    alone, _ = _groups([segments[i] for i in pick], train, prior, 0, 1, [OWN[i] for i in pick])
    n_fill = (1 << 28) + 1000
    rows, letters, seg = _text([segments[i] for i in pick])
    rows = torch.cat([torch.full((n_fill,), -1, dtype=torch.int32, device="cuda"), rows])
    letters = torch.cat([torch.full((n_fill,), kernels.SCORE_SKIP, dtype=torch.uint8, device="cuda"), letters])
    seg = torch.cat([seg[:1], seg + n_fill])
    assert rows.numel() > (1 << 20) * 256
    own = _dev(np.asarray([-1] + [OWN[i] for i in pick], dtype=np.int32))
    scores, short_of = kernels.score_groups(rows, letters, seg, _dev(train), None, None, VANS[:1], own=own)
    scores = scores.cpu().numpy()
    assert not short_of.any() and not scores[0].any()
    assert scores[1:].tobytes() == alone.tobytes() and np.abs(alone).min() > 1


# ------------------------------------------------------------------------------------------- the stream contract
ENTRY = "bear_score_groups_f64"
STREAM_ARG = 15                  # the position of `void *stream` in the entry's declaration


class _StreamSpy(su.Spy):
    """``su.Spy`` that also records, for the entry, the handle in its stream position next to the stream current at the call."""

    def __init__(self, real):
        super().__init__(real)
        self.streams = []

    def __getattr__(self, name):
        fn = su.Spy.__getattr__(self, name)
        if name != ENTRY:
            return fn

        def recorded(*args):
            self.streams.append((su._handle(args[STREAM_ARG]), torch.cuda.current_stream().cuda_stream))
            return fn(*args)
        return recorded


def test_entry_keeps_the_stream_contract_on_a_side_stream(monkeypatch):
    """Class A of tests/test_stream_contract_gpu.py: conditions a-d of ``su.judge`` with a valid decoy table, and the handle in the
    entry's stream position is the side stream's."""
    from bear_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    segments, train, prior = cu.kernel_case(21)
    rows, letters, seg = _text(segments)
    true = dict(rows=rows, letters=letters, c=_dev(train), f=_dev(prior), own=_dev(np.asarray(OWN, dtype=np.int32)))
    decoy_train = np.ascontiguousarray(np.roll(train, 1, axis=1))
    decoy_train[decoy_train < 1000] += 3
    decoy = dict(rows=rows.clone(), letters=letters.clone(), c=_dev(decoy_train), f=torch.full_like(true["f"], 1.0 / 21),
                 own=torch.full_like(true["own"], -1))
    with torch.cuda.device(dev):
        h = su.Harness(dev)
        # torch hands out its pooled streams in turn, and the runtime deals them over its few hardware queues in turn: a side
        # stream that lands on the null stream's queue runs behind the null gate and misses condition d whatever the entry does.
        # The harness took two streams; two more make four, which leaves every later test of the session the queues it has
        # without this one (tests/test_two_sample_gpu.py missed d with two taken, and holds it with none or four)
        spare = [torch.cuda.Stream(dev) for _ in range(2)]
        assert len({s.cuda_stream for s in spare} | {h.side.cuda_stream, h.side2.cuda_stream}) == 4
        su.install_sentinel(monkeypatch)
        spy = _StreamSpy(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", spy)
        try:
            fails = su.judge(h, "score_groups", "A", true, decoy,
                             lambda i: kernels.score_groups(i["rows"], i["letters"], seg, i["c"], i["f"], HS, VANS, own=i["own"]), 1e-11, spy,
                             tol_from="the kernel's bound against mpmath")
        except RuntimeError as e:
            if any(s in str(e) for s in ("illegal memory access", "launch failure", "hipError 7")):
                pytest.exit(f"score_groups: the device faulted ({e}); nothing more is started on it", returncode=3)
            raise
    rec = h.records[-1]
    print(f"score_groups: gate {rec['gate_ms']:.1f} ms, host {rec['host_ms']:.3f} ms, device {rec['dev_ms']:.3f} ms, decoy gap "
          f"{rec['gap']:.3e}, side-stream distance {rec['dist']:.3e}")
    assert not fails, fails
    assert spy.streams and all(got == current for got, current in spy.streams), spy.streams
    assert h.side.cuda_stream != 0 and spy.streams[-1][0] == h.side.cuda_stream
    assert sum(1 for got, _ in spy.streams if got == h.side.cuda_stream) >= 2      # its first use there, and the judged call


# ------------------------------------------------------------------------------------------- the public calls
PUBLIC = {"prot": (2, 2), "dna": (3, 3)}                   # alphabet -> (lag, groups)


def _public_case(alphabet):
    lag, n_groups = PUBLIC[alphabet]
    groups = [tu.sample_seqs(tu.chain(20 + g, alphabet, 1), 200 + g, alphabet, n_seqs=6, length=40, order=1) for g in range(n_groups)]
    fresh = tu.sample_seqs(tu.chain(20, alphabet, 1), 300, alphabet, n_seqs=3, length=55, order=1)
    # (get_bear_probs_seqs, the loop the call is held to, takes no sequence of fewer than lag letters)
    queries = [s for seqs in groups for s in seqs[:2]] + fresh + [groups[0][0][:lag], groups[1][3][:lag + 1], groups[0][5][:lag + 7]]
    return lag, n_groups, groups, queries


def _uniform(W):
    def ar_func(codes):
        return torch.full((codes.shape[0], W), 1.0 / W, dtype=torch.float64, device=codes.device)
    return ar_func


@pytest.mark.parametrize("alphabet", ["prot", "dna"])
def test_public_classify_is_the_per_group_loop(alphabet, monkeypatch):
    lag, n_groups, groups, queries = _public_case(alphabet)
    W = len(tu.LETTERS[alphabet]) + 1
    counter = classify.GroupCounter.from_sequences(groups, lag, alphabet_name=alphabet)
    assert counter.num_groups == n_groups and counter.counts.shape[1:] == (n_groups, W) and not counter.reverse
    hs, vans = np.array([0.05, 3.0]), np.array([0.1, 1.0, 10.0])
    res = classify.classify(counter, queries, ar_func=_uniform(W), h=hs, vans=vans)
    n = len(queries)
    assert res.models == ["bear(h=0.05)", "bear(h=3)", "van(0.1)", "van(1)", "van(10)"]
    assert res.log_marg.shape == res.log_post.shape == (n, n_groups, 5) and res.log_marg.dtype == np.float64
    assert res.best.shape == (n, 5) and res.best.dtype == np.int64
    strings = ["[" * lag + s + "]" for s in queries]
    for g in range(n_groups):
        one = get_var_probs.DeviceCounter.from_sequences(groups[g], lag, reverse=False, alphabet_name=alphabet)
        loop = get_var_probs.get_bear_probs_seqs(None, queries, 0, vans=vans, get_marg=True, lag=lag, alphabet_name=alphabet, counter=one,
                                                 marg_on_device=True)
        assert np.ascontiguousarray(res.log_marg[:, g, 2:]).tobytes() == loop.tobytes(), g
        both = get_var_probs._marg_segments(one, strings, lag, alphabet, hs, _uniform(W), vans).cpu().numpy()
        assert np.ascontiguousarray(res.log_marg[:, g]).tobytes() == both.tobytes(), g
    # against the oracle on the host's own count of the table
    table = cu.count_host(groups, lag, alphabet)
    want, mass = cu.oracle(cu.string_entries(strings, lag, alphabet, table, n_groups, lambda k: np.full(W, 1.0 / W)), hs, vans, W, n_groups)
    _check(res.log_marg, want, mass, f"public {alphabet}")
    assert np.abs(res.log_marg[:n - 3]).min() > 1
    # the posterior, its prior, the arg-max
    assert np.abs(np.exp(res.log_post).sum(1) - 1.0).max() <= 1e-12
    assert np.abs(res.log_post - cu.log_post(res.log_marg)).max() <= 1e-12
    assert np.array_equal(res.best, np.argmax(res.log_post, 1))
    assert (res.best[:2 * n_groups, 3] == np.repeat(np.arange(n_groups), 2)).all()          # its own training sequences, van(1)
    log_prior = np.log(np.arange(1, n_groups + 1) / (n_groups * (n_groups + 1) / 2))
    prior_res = classify.classify(counter, queries, ar_func=_uniform(W), h=hs, vans=vans, log_prior=log_prior)
    assert prior_res.log_marg.tobytes() == res.log_marg.tobytes()
    assert np.abs(prior_res.log_post - cu.log_post(res.log_marg, log_prior)).max() <= 1e-12
    assert np.abs(np.exp(prior_res.log_post).sum(1) - 1.0).max() <= 1e-12
    ruled_out = classify.classify(counter, queries, vans=[1.0], log_prior=[-np.inf] + [0.0] * (n_groups - 1))
    assert (ruled_out.best != 0).all() and np.isneginf(ruled_out.log_post[:, 0]).all()
    # pieces of 2 sequences: the same bits
    calls = []
    score_groups = kernels.score_groups

    def counted(rows, letters, seg, *args, **kw):
        calls.append(seg.numel() - 1)
        return score_groups(rows, letters, seg, *args, **kw)
    monkeypatch.setattr(kernels, "score_groups", counted)
    monkeypatch.setattr(classify, "_pieces", lambda lengths, per_position, budget: [(i, min(i + 2, len(lengths))) for i in range(0, len(lengths), 2)])
    pieces = classify.classify(counter, queries, ar_func=_uniform(W), h=hs, vans=vans)
    assert calls == [2] * (n // 2) + [1] * (n % 2)
    assert pieces.log_marg.tobytes() == res.log_marg.tobytes() and pieces.log_post.tobytes() == res.log_post.tobytes()
    monkeypatch.undo()
    # a counter of one group: the posterior is certain
    single = classify.classify(classify.GroupCounter.from_sequences(groups[:1], lag, alphabet_name=alphabet), queries, vans=[1.0])
    assert not single.log_post.any() and not single.best.any()
    assert np.ascontiguousarray(single.log_marg[:, 0]).tobytes() == np.ascontiguousarray(res.log_marg[:, 0, 3:4]).tobytes()
    assert classify.classify(counter, [], vans=[1.0]).log_marg.shape == (0, n_groups, 1)


@pytest.mark.parametrize("alphabet", ["prot", "dna"])
def test_public_leave_one_out_is_the_table_counted_without_the_sequence(alphabet):
    """``own_group`` on 6 training sequences: each one's own-group marginal has the bits of the marginal under a table counted
    without it; the other groups' are untouched."""
    lag, n_groups, groups, _ = _public_case(alphabet)
    W = len(tu.LETTERS[alphabet]) + 1
    counter = classify.GroupCounter.from_sequences(groups, lag, alphabet_name=alphabet)
    hs, vans = np.array([0.05, 3.0]), np.array([1.0])
    picks = [(g, i) for g in range(n_groups) for i in range(6)][::(6 * n_groups) // 6][:6]
    seqs = [groups[g][i] for g, i in picks]
    own = np.array([g for g, _ in picks])
    assert len(seqs) == 6 and set(own) == set(range(n_groups))
    res = classify.classify(counter, seqs, ar_func=_uniform(W), h=hs, vans=vans, own_group=own)
    plain = classify.classify(counter, seqs, ar_func=_uniform(W), h=hs, vans=vans)
    for k, (g, i) in enumerate(picks):
        without = [list(seqs_g) for seqs_g in groups]
        del without[g][i]
        less = classify.classify(classify.GroupCounter.from_sequences(without, lag, alphabet_name=alphabet), [seqs[k]],
                                 ar_func=_uniform(W), h=hs, vans=vans)
        assert res.log_marg[k].tobytes() == less.log_marg[0].tobytes(), (g, i)
        others = np.arange(n_groups) != g
        assert np.ascontiguousarray(res.log_marg[k, others]).tobytes() == np.ascontiguousarray(plain.log_marg[k, others]).tobytes()
        assert (res.log_marg[k, g] != plain.log_marg[k, g]).all()
    mixed = classify.classify(counter, seqs, ar_func=_uniform(W), h=hs, vans=vans, own_group=np.where(np.arange(6) % 2 == 0, own, -1))
    assert mixed.log_marg[0::2].tobytes() == res.log_marg[0::2].tobytes() and mixed.log_marg[1::2].tobytes() == plain.log_marg[1::2].tobytes()
    # a sequence that its claimed group does not hold: the first one is named
    wrong = (own + 1) % n_groups
    wrong[0] = own[0]
    with pytest.raises(ValueError, match=r"sequence 1 \(.*is not in group %d" % wrong[1]):
        classify.classify(counter, seqs, vans=vans, own_group=wrong)
    if alphabet == "dna":
        both_strands = classify.GroupCounter.from_sequences(groups, lag, alphabet_name="dna", reverse=True)
        assert both_strands.reverse and classify.classify(both_strands, seqs, vans=vans).log_marg.shape == (6, n_groups, 1)
        with pytest.raises(ValueError, match="reverse=True"):
            classify.classify(both_strands, seqs, vans=vans, own_group=own)


def test_public_classify_from_a_dataset():
    from bear_amd import dataloader
    from conftest import YSD1
    data = dataloader.dataloader(YSD1, "dna", 1 << 20, 3)
    counter = classify.GroupCounter.from_dataset(data, cols=[2, 0])
    assert counter.num_groups == 2 and counter.lag == data.lag
    clean = [k for k in (bytes(k).decode() for k in data.kmers[:200]) if "[" not in k]
    seqs = [clean[i] + clean[i + 1] for i in range(8)] + ["ACGTTGCAAGGCTTAACG"]
    res = classify.classify(counter, seqs, vans=[0.1, 1.0], no_ends=True)
    for g, col in enumerate((2, 0)):
        one = get_var_probs.DeviceCounter.from_dataset(data, col)
        loop = get_var_probs.get_bear_probs_seqs(None, seqs, 0, vans=[0.1, 1.0], get_marg=True, lag=data.lag, alphabet_name="dna", counter=one,
                                                 marg_on_device=True, no_ends=True)
        assert np.ascontiguousarray(res.log_marg[:, g]).tobytes() == loop.tobytes()
    on_dev = dataloader.DeviceCountDataset(torch.from_numpy(data.kmers).to("cuda"), torch.from_numpy(data.counts.view(np.int32)).to("cuda"), "dna", 400)
    again = classify.classify(classify.GroupCounter.from_dataset(on_dev, cols=[2, 0]), seqs, vans=[0.1, 1.0], no_ends=True)
    assert again.log_marg.tobytes() == res.log_marg.tobytes() and np.abs(res.log_marg[-1]).min() > 1


# ------------------------------------------------------------------------------------------- the statistical case
@pytest.mark.parametrize("alphabet", ["dna", "prot"])
@pytest.mark.parametrize("lag", cu.STAT_LAGS)
def test_statistical_case_follows_the_oracle(alphabet, lag):
    """Two order-1 chains per alphabet, 200 training and 100 held-out sequences of 60 letters per group, the vanilla model van(1):
    ``best`` is the oracle's arg-max for every held-out sequence whose oracle margin exceeds 1e-6 (none is excluded, at most 1 % may
    be).  The oracle's accuracy on the held-out set: dna lag 1 0.995, dna lag 2 1.0, prot lag 1 1.0, prot lag 2 1.0."""
    train, held = cu.stat_case(alphabet)
    want, margin, accuracy = cu.stat_oracle(alphabet, lag)
    decided = margin > 1e-6
    assert (~decided).mean() <= 0.01 and accuracy >= 0.9
    counter = classify.GroupCounter.from_sequences(train, lag, alphabet_name=alphabet)
    res = classify.classify(counter, [s for seqs in held for s in seqs], vans=cu.STAT_VANS)
    assert res.best.shape == (200, 1)
    assert np.array_equal(res.best[decided, 0], np.argmax(want[decided, :, 0], 1))
    print(f"classify {alphabet} lag {lag}: oracle accuracy {accuracy:.3f}, device accuracy "
          f"{(res.best[:, 0] == np.repeat([0, 1], 100)).mean():.3f}, {int((~decided).sum())} excluded")
