"""GPU tests of the segmentation (kernels_segment.h, kernels.emit_groups, kernels.hmm_groups, bear_amd.classify.position_log_probs and
.segment): the emissions against the formula at 50 digits at both widths; the chain against both recurrences at 50 digits (a
longdouble twin at sixteen states) over one, two and several chunks; a segment's bits alone, inside a text and from the
deterministic library; the stream contract of include/bear_hip.h on a side stream for both entries (their stream is not their
last parameter, so tests/test_stream_contract_gpu.py does not see them: same harness, here); the public calls; a statistical case.

The bounds.  Emissions: ``|got - want| <= 1e-11 * (|log a_l| + |log A|)``, a_l and A the float64 values the header defines (where both
are next to 1 their own roundings are all there is of the scale: the value in exact arithmetic is held to the bound plus those).  Chain: ``1e-11 * mass``, ``mass = sum_t max_g |e_t(g)| +
(T - 1) max|log_trans| + max|log_start|`` -- every step adds at most one rounding of a value no larger than the mass, and
T * 2^-53 < 1e-11 for the T < 9e4 used here.  The largest ratios observed on an MI355X are printed per case and recorded in
DESIGN.md."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classify_util as cu
import segment_util as sg
import stream_util as su
import two_sample_util as tu
from bear_amd import classify, kernels
from conftest import ROOT

pytestmark = pytest.mark.gpu

C = kernels.HMM_CHUNK
RTOL = sg.RTOL


def _dev(a):
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _hmm(emit, seg, lt, ls, want_post=True):
    """``kernels.hmm_groups`` on host arrays -> (log_evidence, log_best, path, log_post or None) as NumPy arrays."""
    n_t, n_seg, S = emit.shape[0], len(seg) - 1, emit.shape[1]
    out = kernels.hmm_groups(_dev(emit), _dev(np.asarray(seg, dtype=np.int64)), lt, ls, want_post=want_post)
    assert all(o.is_cuda for o in out if o is not None) and out[2].dtype == torch.uint8 and out[2].shape == (n_t,)
    assert out[0].shape == out[1].shape == (n_seg,) and (out[3] is None) == (not want_post) and (out[3] is None or out[3].shape == (n_t, S))
    return tuple(None if o is None else o.cpu().numpy() for o in out)


# ------------------------------------------------------------------------------------------- 1. the emissions
@pytest.mark.parametrize("which", range(len(sg.EMIT_CASES)))
@pytest.mark.parametrize("W", [5, 21])
def test_emission_against_the_oracle(W, which):
    rows, letters, train, prior, hs, vans, want, scale, exact = sg.emit_case(W, which)
    K, G, _ = train.shape
    n_t, M = rows.size, len(hs) + len(vans)
    assert n_t == 4097 > 16 * 256 and n_t % 256                          # several blocks, a ragged last one
    none = ~((rows >= 0) & (rows < K) & (letters < W))
    assert 0.05 < none.mean() < 0.15 and (rows[none] >= K).any() and (rows[none] < 0).any() and ((letters == 0xFF) & (rows >= 0) & (rows < K)).any()
    got = kernels.emit_groups(_dev(rows), _dev(letters), _dev(train), _dev(prior), hs, vans)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (M, n_t, G)
    got = got.cpu().numpy()
    err = np.abs(got - want)
    ratio = float((err / np.where(scale > 0, scale, 1.0)).max())
    print(f"segment emission W={W} K={K} G={G} M={M}: largest |got - want| / (|log a_l| + |log A|) = {ratio:.3e} (bound {RTOL:.0e})")
    assert np.all(err <= RTOL * scale), ratio
    assert np.all(np.abs(got - exact) <= RTOL * scale + sg.input_rounding(W) * (scale > 0))      # ... and next to exact arithmetic
    assert np.array_equal(scale == 0, np.broadcast_to(none[None, :, None], scale.shape))
    assert not got[:, none, :].any() and not np.signbit(got[:, none, :]).any()         # no transition: exactly 0.0
    assert (got[:, ~none, :] < 0).all()
    # the vanilla models alone, without a prior: the bits of their planes
    alone = kernels.emit_groups(_dev(rows), _dev(letters), _dev(train), None, None, vans).cpu().numpy()
    assert alone.tobytes() == np.ascontiguousarray(got[len(hs):]).tobytes()
    assert kernels.emit_groups(_dev(rows[:0]), _dev(letters[:0]), _dev(train), None, None, vans).shape == (len(vans), 0, G)


# ------------------------------------------------------------------------------------------- 2. the chain
@pytest.mark.parametrize("name", ["sticky", "dense", "left_to_right"])
@pytest.mark.parametrize("S", [1, 2, 3, 16])
def test_chain_against_the_oracle(S, name):
    emit, seg, lt, ls, want, mass = sg.chain_case(S, name, C)
    assert min(float(w["gap"].min()) if w["gap"].size else np.inf for w in want) > sg.MIN_GAP
    ev, best, path, post = _hmm(emit, seg, lt, ls)
    worst = 0.0
    for i, (w, m) in enumerate(zip(want, mass)):
        a, b = seg[i], seg[i + 1]
        for k, got in (("log_evidence", ev[i]), ("log_best", best[i])):
            worst = max(worst, abs(got - w[k]) / m if m else 0.0)        # (no step and a start of 0: a mass of 0, equal bits)
            assert abs(got - w[k]) <= RTOL * m, (i, k, got, w[k])
        assert np.array_equal(path[a:b], w["path"]), (i, int((path[a:b] != w["path"]).sum()))          # every position
        finite = np.isfinite(w["log_post"])
        assert np.array_equal(post[a:b][~finite], w["log_post"][~finite])                                 # exactly -inf where it is
        if finite.any():
            err = float(np.abs(post[a:b][finite] - w["log_post"][finite]).max())
            worst = max(worst, err / m)
            assert err <= RTOL * m, (i, err, m)
    print(f"segment chain S={S} {name}: largest error / mass = {worst:.3e} (bound {RTOL:.0e})")
    if name == "left_to_right" and S > 1:
        assert np.isneginf(post).any()
    # without the posterior: the same scalars and path
    ev2, best2, path2, none = _hmm(emit, seg, lt, ls, want_post=False)
    assert none is None and ev2.tobytes() == ev.tobytes() and best2.tobytes() == best.tobytes() and path2.tobytes() == path.tobytes()


def test_chain_without_a_step_and_without_a_path():
    lt, ls = sg.chains(3)["dense"]
    ev, best, path, post = _hmm(np.zeros((0, 3)), [0, 0, 0], lt, ls)                      # segments, and no step anywhere
    want = sg.chain_oracle(np.zeros((0, 3)), lt, ls)
    assert np.abs(ev - want["log_evidence"]).max() <= 1e-15 * abs(want["log_evidence"]) + 1e-15 and (best == ls.max()).all()
    assert kernels.hmm_groups(_dev(np.zeros((0, 3))), _dev(np.zeros(1, dtype=np.int64)), lt, ls)[0].shape == (0,)      # no segment
    # a chain that must alternate from state 0 while the second step's emission rules state 1 out: no path is left.  Between two
    # live segments, at one chunk and beyond
    NEG = float("-inf")
    lt2, ls2 = np.array([[NEG, 0.0], [0.0, NEG]]), np.array([0.0, NEG])
    rng = np.random.default_rng(3)
    live = rng.normal(-2.0, 1.5, (C + 9, 2))
    for T in (3, C + 40):
        dead = live[:T].copy()
        dead[1, 1] = NEG
        emit = np.concatenate([live[:7], dead, live[:C + 9]])
        seg = [0, 7, 7 + T, 7 + T + C + 9]
        ev, best, path, post = _hmm(emit, seg, lt2, ls2)
        assert ev[1] == NEG and best[1] == NEG and np.isnan(post[7:7 + T]).all() and (path[7:7 + T] == 255).all()
        for i, (a, b) in enumerate(((0, 7), (7 + T, seg[3]))):
            want = sg.chain_oracle(emit[a:b], lt2, ls2)
            assert np.array_equal(path[a:b], want["path"]) and abs(ev[2 * i] - want["log_evidence"]) <= RTOL * sg.chain_mass(emit[a:b], lt2, ls2)


# ------------------------------------------------------------------------------------------- 3. a segment's bits are its content's
BITS_CASES = [(3, "dense", 6), (16, "sticky", 2), (2, "left_to_right", 6)]         # (S, chain, the longest segment of the case)


def _bits_runs(S, name, which):
    """The segment alone, and at another offset between other segments -> the two runs' four outputs for that segment."""
    emit, seg, lt, ls, _, _ = sg.chain_case(S, name, C)
    parts = [emit[a:b] for a, b in zip(seg[:-1], seg[1:])]
    assert len(parts[which]) == (C + 1 if S == 16 else 3 * C + 17)
    alone = _hmm(parts[which], [0, len(parts[which])], lt, ls)
    order = [which - 1, 1, which, 1, which - 1] if S == 16 else [5, 1, which, 4, 2]
    seg2 = np.concatenate([[0], np.cumsum([len(parts[i]) for i in order])])
    ev, best, path, post = _hmm(np.concatenate([parts[i] for i in order]), seg2, lt, ls)
    a, b = seg2[2], seg2[3]
    assert a % C and a != seg[which]
    return alone, (ev[2:3], best[2:3], path[a:b], post[a:b])


@pytest.mark.parametrize("S,name,which", BITS_CASES)
def test_a_segment_has_the_same_bits_alone_as_inside_the_text(S, name, which):
    emit, seg, lt, ls, _, _ = sg.chain_case(S, name, C)
    ev, best, path, post = _hmm(emit, seg, lt, ls)
    a, b = seg[which], seg[which + 1]
    whole = (ev[which:which + 1], best[which:which + 1], path[a:b], post[a:b])
    alone, between = _bits_runs(S, name, which)
    for x, y, z in zip(whole, alone, between):
        assert np.ascontiguousarray(x).tobytes() == y.tobytes() == np.ascontiguousarray(z).tobytes()
    assert np.isfinite(alone[0]).all() and len(set(alone[2].tolist())) > 1


_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from bear_amd import _lib
import segment_util as sg
import test_segment_gpu as t
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
out = {}
for S, name, which in t.BITS_CASES:
    alone, _ = t._bits_runs(S, name, which)
    for k, v in zip(("ev", "best", "path", "post"), alone):
        out[f"{k}_{S}"] = v
rows, letters, train, prior, hs, vans = sg.emit_case(21, 0)[:6]
out["emit"] = t.kernels.emit_groups(t._dev(rows), t._dev(letters), t._dev(train), t._dev(prior), hs, vans).cpu().numpy()
np.savez(sys.argv[2], **out)
"""


def test_deterministic_library_returns_the_same_bits(tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    here = {}
    for S, name, which in BITS_CASES:
        alone, _ = _bits_runs(S, name, which)
        for k, v in zip(("ev", "best", "path", "post"), alone):
            here[f"{k}_{S}"] = v
    rows, letters, train, prior, hs, vans = sg.emit_case(21, 0)[:6]
    here["emit"] = kernels.emit_groups(_dev(rows), _dev(letters), _dev(train), _dev(prior), hs, vans).cpu().numpy()
    script = tmp_path / "det_segment.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npz")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    there = np.load(tmp_path / "det.npz")
    assert set(there.files) == set(here)
    for k, v in here.items():
        assert there[k].shape == v.shape and there[k].tobytes() == v.tobytes(), k


# ------------------------------------------------------------------------------------------- 4. the stream contract
STREAM_ARG = {"bear_score_emit_groups_f64": 12, "bear_hmm_groups_f64": 7}      # the position of `void *stream` in the declarations


class _StreamSpy(su.Spy):
    """``su.Spy`` that also records, for the two entries, the handle in their stream position next to the stream current at the call."""

    def __init__(self, real):
        super().__init__(real)
        self.streams = {name: [] for name in STREAM_ARG}

    def __getattr__(self, name):
        fn = su.Spy.__getattr__(self, name)
        if name not in STREAM_ARG:
            return fn

        def recorded(*args):
            self.streams[name].append((su._handle(args[STREAM_ARG[name]]), torch.cuda.current_stream().cuda_stream))
            return fn(*args)
        return recorded


def _stream_cases():
    rows, letters, train, prior, hs, vans = sg.emit_case(21, 0)[:6]
    decoy_train = np.ascontiguousarray(np.roll(train, 1, axis=1))
    decoy_train[decoy_train < 1000] += 3
    true = dict(rows=_dev(rows), letters=_dev(letters), c=_dev(train), f=_dev(prior))
    decoy = dict(rows=true["rows"].clone(), letters=true["letters"].clone(), c=_dev(decoy_train), f=torch.full_like(true["f"], 1.0 / 21))
    yield ("bear_score_emit_groups_f64", "emit_groups", true, decoy,
           lambda i: kernels.emit_groups(i["rows"], i["letters"], i["c"], i["f"], hs, vans), None)
    lt, ls = sg.chains(3)["dense"]
    rng = np.random.default_rng(77)
    seg = np.concatenate([[0], np.cumsum([0, 1, 7, 64, 33, 0, 50])]).astype(np.int64)             # segments of one chunk
    emit, other = rng.normal(-2.0, 1.5, (seg[-1], 3)), rng.normal(-2.0, 1.5, (seg[-1], 3))
    short_seg = _dev(seg)
    yield ("bear_hmm_groups_f64", "hmm_groups", dict(e=_dev(emit)), dict(e=_dev(other)), lambda i: kernels.hmm_groups(i["e"], short_seg, lt, ls), None)
    # Segments beyond one chunk: the matrix, carry and normalise launches, the block items of the chunk kernel and the pool
    # allocations behind them.  The harness's null gate lasts NULL_FACTOR = 3 times the side stream's work as timed on an idle
    # device: it allows for work that slows threefold while the two gates' matrix products share the device with it.  These
    # kernels are one wave a chunk stepping through up to 512 DEPENDENT steps: such a wave issues one instruction at a time, and
    # on a SIMD it shares with the gates' waves (up to 8 waves a SIMD, issued in turn) it gets as little as one slot in eight --
    # an eightfold slow-down is within what sharing alone does, and the side gate in front of it slows twofold besides.  So this
    # case gets 12 = 8 and half as much again.  The factor cannot hide what condition d is for: an entry that waits for the whole
    # device waits for the null gate itself, however long that is.
    emit, seg, lt2, ls2, _, _ = sg.chain_case(3, "dense", C)
    assert (np.diff(seg) > C).any() and emit.shape[0] > C
    long_seg = _dev(seg)
    other = np.random.default_rng(78).normal(-2.0, 1.5, emit.shape)
    yield ("bear_hmm_groups_f64", "hmm_groups beyond one chunk", dict(e=_dev(emit)), dict(e=_dev(other)),
           lambda i: kernels.hmm_groups(i["e"], long_seg, lt2, ls2), 12)


def test_entries_keep_the_stream_contract_on_a_side_stream(monkeypatch):
    """Class A of tests/test_stream_contract_gpu.py for both entries -- the chain with segments of one chunk and with segments beyond
    one (``_stream_cases`` says why that case alone has a longer null gate): conditions a-d of ``su.judge`` with a valid decoy,
    equal bits to the default-stream run, and the handle in each entry's stream position is the side stream's."""
    from bear_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        cases = list(_stream_cases())
        h = su.Harness(dev)
        # (tests/test_classify_gpu.py says why: four streams taken leave every later test of the session the queues it has)
        spare = [torch.cuda.Stream(dev) for _ in range(2)]
        assert len({s.cuda_stream for s in spare} | {h.side.cuda_stream, h.side2.cuda_stream}) == 4
        su.install_sentinel(monkeypatch)
        spy = _StreamSpy(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", spy)
        harness_factor = su.NULL_FACTOR
        for entry, name, true, decoy, call, null_factor in cases:
            spy.streams[entry].clear()
            monkeypatch.setattr(su, "NULL_FACTOR", null_factor or harness_factor)      # (for this case alone)
            try:
                fails = su.judge(h, name, "A", true, decoy, call, 0.0, spy, tol_from="no atomics: equal bits")
            except RuntimeError as e:
                if any(s in str(e) for s in ("illegal memory access", "launch failure", "hipError 7")):
                    pytest.exit(f"{name}: the device faulted ({e}); nothing more is started on it", returncode=3)
                raise
            rec = h.records[-1]
            print(f"{name}: null factor {su.NULL_FACTOR}, gate {rec['gate_ms']:.1f} ms, host {rec['host_ms']:.3f} ms, device {rec['dev_ms']:.3f} ms, decoy gap "
                  f"{rec['gap']:.3e}, side-stream distance {rec['dist']:.3e}")
            assert not fails, (name, fails)
            seen = spy.streams[entry]
            assert seen and all(got == current for got, current in seen), (name, seen)
            assert h.side.cuda_stream != 0 and seen[-1][0] == h.side.cuda_stream
            assert sum(1 for got, _ in seen if got == h.side.cuda_stream) >= 2      # its first use there, and the judged call


# ------------------------------------------------------------------------------------------- 5. the public calls
PUBLIC = {"prot": (2, 2), "dna": (3, 3)}                   # alphabet -> (lag, groups)


def _public_case(alphabet):
    lag, n_groups = PUBLIC[alphabet]
    groups = [tu.sample_seqs(tu.chain(20 + g, alphabet, 1), 200 + g, alphabet, n_seqs=6, length=40, order=1) for g in range(n_groups)]
    chimera = groups[0][0][:25] + groups[1][0][:30] + groups[0][1][:20]
    queries = [s for seqs in groups for s in seqs[:2]] + [chimera, groups[0][0][:lag], "", groups[1][3][:lag + 1]]
    return lag, n_groups, groups, queries


def _uniform(W):
    def ar_func(codes):
        return torch.full((codes.shape[0], W), 1.0 / W, dtype=torch.float64, device=codes.device)
    return ar_func


def _distinct_prefix(s, lag):
    """The longest prefix of ``s`` whose padded string holds every context once."""
    for n in range(len(s), 0, -1):
        t = "[" * lag + s[:n] + "]"
        contexts = [t[p - lag:p] for p in range(lag, len(t))]
        if len(set(contexts)) == len(contexts):
            return s[:n]
    return ""


@pytest.mark.parametrize("alphabet", ["prot", "dna"])
def test_public_calls(alphabet, monkeypatch):
    lag, n_groups, groups, queries = _public_case(alphabet)
    W = len(tu.LETTERS[alphabet]) + 1
    counter = classify.GroupCounter.from_sequences(groups, lag, alphabet_name=alphabet)
    hs, vans = np.array([0.05, 3.0]), np.array([0.1, 1.0])
    plp = classify.position_log_probs(counter, queries, ar_func=_uniform(W), h=hs, vans=vans)
    counts = [len(s) + 1 for s in queries]                   # a sequence's letters, then its stop
    assert plp.models == ["bear(h=0.05)", "bear(h=3)", "van(0.1)", "van(1)"]
    assert plp.offsets.dtype == np.int64 and plp.offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert plp.log_prob.dtype == np.float64 and plp.log_prob.shape == (sum(counts), n_groups, 4)
    # against the oracle on the host's own count of the table
    strings = ["[" * lag + s + "]" for s in queries]
    table = cu.count_host(groups, lag, alphabet)
    want, scale = sg.string_emissions(strings, lag, alphabet, table, n_groups, hs, vans, lambda k: np.full(W, 1.0 / W))
    err = np.abs(plp.log_prob - want)
    print(f"segment public {alphabet}: largest |got - want| / (|log a_l| + |log A|) = {float((err / scale).max()):.3e} (bound {RTOL:.0e})")
    assert np.all(err <= RTOL * scale) and (plp.log_prob < 0).all()
    # a sequence whose k-mers are all distinct: its rows add up to its marginal
    distinct = [_distinct_prefix(s, lag) for s in queries[:2 * n_groups]]
    assert min(len(s) for s in distinct) >= lag + 3
    rows = classify.position_log_probs(counter, distinct, ar_func=_uniform(W), h=hs, vans=vans)
    marg = classify.classify(counter, distinct, ar_func=_uniform(W), h=hs, vans=vans).log_marg
    _, scale_d = sg.string_emissions(["[" * lag + s + "]" for s in distinct], lag, alphabet, table, n_groups, hs, vans, lambda k: np.full(W, 1.0 / W))
    worst = 0.0
    for i in range(len(distinct)):
        a, b = rows.offsets[i], rows.offsets[i + 1]
        # the marginal's brackets are log a_l and -log A here: its L1 mass is the sum of the rows' scales
        diff, mass = np.abs(rows.log_prob[a:b].sum(0) - marg[i]), scale_d[a:b].sum(0)
        worst = max(worst, float((diff / mass).max()))
        assert np.all(diff <= RTOL * mass), (i, worst)
    print(f"segment public {alphabet}: largest |sum of rows - log_marg| / mass = {worst:.3e} (bound {RTOL:.0e})")
    # no_ends: the letters behind the first lag
    bare = classify.position_log_probs(counter, queries[:3], vans=vans, no_ends=True)
    assert bare.offsets.tolist() == np.concatenate([[0], np.cumsum([len(s) - lag for s in queries[:3]])]).tolist()
    for i, s in enumerate(queries[:3]):                      # the same transitions as with ends, less the padded ones and the stop
        a = plp.offsets[i]
        assert bare.log_prob[bare.offsets[i]:bare.offsets[i + 1]].tobytes() == np.ascontiguousarray(plp.log_prob[a + lag:a + len(s), :, 2:]).tobytes()
    # segment is kernels.hmm_groups on those emissions
    for model, kw in ((1, dict(switch=0.02)), (3, dict(log_trans=sg.chains(n_groups)["dense"][0], log_start=sg.chains(n_groups)["dense"][1]))):
        res = classify.segment(counter, queries, ar_func=_uniform(W), h=hs, vans=vans, model=model, **kw)
        lt, ls = sg.sticky(n_groups, 0.02) if "switch" in kw else (kw["log_trans"], kw["log_start"])
        emit = _dev(np.ascontiguousarray(plp.log_prob[:, :, model]))
        ev, best, path, post = (o.cpu().numpy() for o in kernels.hmm_groups(emit, _dev(plp.offsets), lt, ls))
        assert res.model == plp.models[model] and res.offsets.tolist() == plp.offsets.tolist()
        assert res.path.dtype == np.uint8 and res.path.tobytes() == path.tobytes() and res.log_post.tobytes() == post.tobytes()
        assert res.log_evidence.tobytes() == ev.tobytes() and res.log_best.tobytes() == best.tobytes()
        assert res.log_post.shape == (sum(counts), n_groups) and res.log_best.shape == res.log_evidence.shape == (len(queries),)
        assert (res.log_best <= res.log_evidence).all() and np.abs(np.exp(res.log_post).sum(1) - 1.0).max() <= 1e-12
        for i, n in enumerate(counts):                       # the stretches tile [0, transitions)
            runs = res.runs(i)
            assert runs[0][0] == 0 and runs[-1][1] == n and all(a[1] == b[0] and a[2] != b[2] for a, b in zip(runs, runs[1:]))
            assert all(np.all(res.path[res.offsets[i] + a:res.offsets[i] + b] == g) for a, b, g in runs)
        bare = classify.segment(counter, queries, ar_func=_uniform(W), h=hs, vans=vans, model=model, posterior=False, **kw)
        assert bare.log_post is None and bare.path.tobytes() == res.path.tobytes() and bare.log_evidence.tobytes() == res.log_evidence.tobytes()
    sticky = classify.segment(counter, queries, vans=[1.0], switch=0.02)
    own = np.repeat(np.arange(n_groups), 2)
    assert all(np.bincount(sticky.path[sticky.offsets[i]:sticky.offsets[i + 1]], minlength=n_groups).argmax() == own[i] for i in range(2 * n_groups))
    assert len(sticky.runs(2 * n_groups)) >= 3               # the chimera: group 0, group 1, group 0
    # a piece budget of one sequence: the same bits
    monkeypatch.setattr(classify, "_pieces", lambda lengths, per_position, budget: [(i, i + 1) for i in range(len(lengths))])
    pieces = classify.segment(counter, queries, vans=[1.0], switch=0.02)
    plp_pieces = classify.position_log_probs(counter, queries, ar_func=_uniform(W), h=hs, vans=vans)
    monkeypatch.undo()
    assert pieces.path.tobytes() == sticky.path.tobytes() and pieces.log_post.tobytes() == sticky.log_post.tobytes()
    assert pieces.log_evidence.tobytes() == sticky.log_evidence.tobytes() and pieces.log_best.tobytes() == sticky.log_best.tobytes()
    assert plp_pieces.log_prob.tobytes() == plp.log_prob.tobytes()
    none = classify.segment(counter, [], vans=[1.0], switch=0.02)
    assert none.path.shape == (0,) and none.log_post.shape == (0, n_groups) and none.offsets.tolist() == [0]


# ------------------------------------------------------------------------------------------- 6. the statistical case
@pytest.mark.parametrize("alphabet", ["dna", "prot"])
@pytest.mark.parametrize("lag", cu.STAT_LAGS)
def test_statistical_case_follows_the_oracle(alphabet, lag):
    """40 chimeras of 600 letters of two order-1 chains (``sg.stat_chimeras``), a table of 200 training sequences per group, van(1)
    and a switch probability of 0.005: ``path`` is the oracle's at every transition (its smallest gap is 2e-3) and so reaches its
    accuracy -- dna lag 1 / 2 0.983 / 0.985, prot lag 1 / 2 0.995 / 0.993."""
    train, _ = cu.stat_case(alphabet)
    seqs, truth = sg.stat_chimeras(alphabet)
    paths, gap, accuracy = sg.stat_oracle(alphabet, lag)
    assert gap > sg.MIN_GAP and accuracy >= 0.9
    counter = classify.GroupCounter.from_sequences(train, lag, alphabet_name=alphabet)
    res = classify.segment(counter, seqs, vans=cu.STAT_VANS, switch=sg.STAT_SWITCH)
    assert res.path.shape == (sg.STAT_N * (sg.STAT_LEN + 1),)
    assert np.array_equal(res.path, np.concatenate(paths))
    labels = np.concatenate([np.concatenate([t, t[-1:]]) for t in truth])
    device_accuracy = float((res.path == labels).mean())
    print(f"segment {alphabet} lag {lag}: oracle accuracy {accuracy:.4f}, device accuracy {device_accuracy:.4f}, smallest gap {gap:.2e}")
    assert abs(device_accuracy - accuracy) < 1e-12
