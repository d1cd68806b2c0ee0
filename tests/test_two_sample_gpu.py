"""GPU tests of the two-sample and goodness-of-fit Bayes factors (kernels_twosample.h, kernels.two_sample, bear_amd.hypothesis): the
kernel against the formulas evaluated with mpmath at 50 digits (tests/two_sample_util.py) at both widths, its structure in equal
bits, an existing entry, the grid stride, sixteen models, the stream contract of include/bear_hip.h on a side stream (the entry's
stream is not its last parameter, so tests/test_stream_contract_gpu.py does not see it: same harness, here) and the public calls.

The bound everywhere: ``|got - want| <= 1e-11 * mass``, ``mass`` the L1 sum of the lgamma brackets (resp. of the ``c log p`` terms)
behind that output -- the figure of tests/test_marg_gpu.py for this item routine and these terms.  The largest ratio observed on an
MI355X is printed per case and recorded in DESIGN.md 4.13."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stream_util as su
import two_sample_util as tu
from bear_amd import ar_funcs, dataloader, hypothesis, kernels, summarize
from conftest import ROOT, YSD1
from two_sample_util import HS, RTOL, VANS

pytestmark = pytest.mark.gpu

N_BIG = 4097
WIDTHS = (5, 21)


def _dev(x):
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def _ratio(got, want, mass):
    return float((np.abs(got - want) / np.where(mass > 0, mass, 1.0)).max()) if got.size else 0.0


def _check(got, want, mass, what, rtol=RTOL):
    ratio = _ratio(got, want, mass)
    print(f"two-sample {what}: largest |got - want| / mass = {ratio:.3e} (bound {rtol:.0e})")
    assert got.shape == want.shape and np.all(np.abs(got - want) <= rtol * mass), (what, ratio)


@pytest.fixture(scope="module")
def base():
    """Per width the rows of every kind and their oracle, computed once."""
    out = {}
    for W in WIDTHS:
        a, b, prior = tu.base_rows(W)
        out[W] = (a, b, prior, tu.oracle_rows(a, b, prior, HS, VANS))
    return out


def _table(base, W, n, seed=0):
    a, b, prior, rows = base[W]
    idx = tu.table_index(len(a), n, seed)
    return idx, a[idx], b[idx], prior[idx]


def _run(a, b, prior, hs=HS, vans=VANS, want_ar=True, want_rows=True):
    out, out_ar, terms = kernels.two_sample(_dev(a), _dev(b), None if prior is None else _dev(prior), hs, vans, want_ar=want_ar,
                                            want_rows=want_rows)
    return tuple(None if t is None else t.cpu().numpy() for t in (out, out_ar, terms))


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("size", ["1", "tile-1", "tile", "tile+1", "4097"])
def test_kernel_against_mpmath(base, W, size):
    tile = kernels.TWO_SAMPLE_TILE[W]
    n = {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "4097": N_BIG}[size]
    rows = base[W][3]
    idx, a, b, prior = _table(base, W, n)
    if n > 1:
        assert set(idx.tolist()) == set(range(len(base[W][0])))                # rows of every kind
    out, out_ar, terms = _run(a, b, prior)
    want, mass, want_ar, mass_ar = tu.oracle_sums(rows, idx)
    _check(out, want, mass, f"W={W} n={n} sums")
    _check(out_ar, want_ar, mass_ar, f"W={W} n={n} AR log-likelihoods")
    _check(terms, tu.as_float(rows[0][idx][:, :, 3]), tu.as_float(rows[1][idx][:, :, 3]), f"W={W} n={n} row terms")
    one_side = (a.astype(np.uint64).sum(1) == 0) | (b.astype(np.uint64).sum(1) == 0)
    assert terms.shape == (n, 6) and not terms[one_side].view(np.int64).any()      # exactly +0.0 (the bit pattern) where a side is empty
    if n > 1:
        assert one_side.any() and np.abs(terms[~one_side]).min() > 0 and np.abs(out).min() > 1.0
    again = _run(a, b, prior)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((out, out_ar, terms), again))     # the same call twice: equal bits


@pytest.mark.parametrize("W", WIDTHS)
def test_structure_in_equal_bits(base, W):
    _, a, b, prior = _table(base, W, N_BIG, seed=1)
    out, out_ar, terms = _run(a, b, prior)
    s_out, s_ar, s_terms = _run(b, a, prior)                                    # swapped samples
    assert s_out[:, 0].tobytes() == out[:, 1].tobytes() and s_out[:, 1].tobytes() == out[:, 0].tobytes()
    assert s_out[:, 2:].tobytes() == out[:, 2:].tobytes() and s_terms.tobytes() == terms.tobytes()
    assert s_ar[::-1].tobytes() == out_ar.tobytes()
    e_out, e_ar, e_terms = _run(a, np.zeros_like(b), prior)                     # an empty second sample
    assert not e_out[:, 3].view(np.int64).any() and not e_out[:, 1].any() and not e_terms.view(np.int64).any() and e_ar[1] == 0.0
    assert e_out[:, 2].tobytes() == e_out[:, 0].tobytes() == out[:, 0].tobytes() and e_ar[0] == out_ar[0]
    for want_ar, want_rows in ((False, True), (True, False), (False, False)):  # omitted outputs do not change the others
        o, r, t = _run(a, b, prior, want_ar=want_ar, want_rows=want_rows)
        assert o.tobytes() == out.tobytes() and (r is None) != want_ar and (t is None) != want_rows
        assert (r is None or r.tobytes() == out_ar.tobytes()) and (t is None or t.tobytes() == terms.tobytes())
    v_out, _, v_terms = _run(a, b, None, hs=None, want_ar=False)                # vanilla models alone, no prior rows
    assert v_out.tobytes() == out[3:].tobytes() and v_terms.tobytes() == np.ascontiguousarray(terms[:, 3:]).tobytes()
    z_out, z_ar, z_terms = _run(a[:0], b[:0], prior[:0])                        # no rows: zeros
    assert z_out.shape == (6, 4) and not z_out.any() and not z_ar.any() and z_terms.shape == (0, 6)


_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from bear_amd import _lib
import test_two_sample_gpu as t
import two_sample_util as tu
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
a, b, prior = tu.base_rows(21)
idx = tu.table_index(len(a), t.N_BIG, 1)
out, out_ar, terms = t._run(a[idx], b[idx], prior[idx])
np.savez(sys.argv[2], out=out, out_ar=out_ar, terms=terms)
"""


def test_deterministic_library_returns_the_same_bits(base, tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    _, a, b, prior = _table(base, 21, N_BIG, seed=1)
    here = _run(a, b, prior)
    script = tmp_path / "det_two_sample.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npz")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    there = np.load(tmp_path / "det.npz")
    for name, x in zip(("out", "out_ar", "terms"), here):
        assert there[name].shape == x.shape and there[name].tobytes() == x.tobytes(), name


def test_vanilla_marginal_is_the_bmm_entry(base):
    """M_a of the vanilla models is the sum bear_bmm_f64 forms with another kernel: each within 1e-11 of the mass, so 2e-11 apart."""
    idx, a, b, prior = _table(base, 5, N_BIG)
    out, _, _ = _run(a, b, prior, want_ar=False, want_rows=False)
    bmm = kernels.bmm(_dev(a), VANS).cpu().numpy()
    _, mass, _, _ = tu.oracle_sums(base[5][3], idx)
    _check(out[3:, 0], bmm, mass[3:, 0], "M_a of the vanilla models against kernels.bmm", rtol=2 * RTOL)


@pytest.mark.parametrize("W", WIDTHS)
def test_grid_stride(base, W):
    """More tiles than a launch has blocks (blocks per CU x 256 CUs): the 4097-row table repeated sums to the repeat count times its
    oracle."""
    idx, a, b, prior = _table(base, W, N_BIG)
    reps = kernels.TWO_SAMPLE_BLOCKS_PER_CU * 256 * kernels.TWO_SAMPLE_TILE[W] // N_BIG + 2
    assert reps * N_BIG > kernels.TWO_SAMPLE_BLOCKS_PER_CU * 256 * kernels.TWO_SAMPLE_TILE[W] + kernels.TWO_SAMPLE_TILE[W]
    ad, bd, pd = (_dev(x).repeat(reps, 1) for x in (a, b, prior))
    out, out_ar, terms = kernels.two_sample(ad, bd, pd, HS, VANS, want_ar=True, want_rows=True)
    want, mass, want_ar, mass_ar = tu.oracle_sums(base[W][3], idx)
    _check(out.cpu().numpy(), reps * want, reps * mass, f"W={W} {reps} x {N_BIG} rows, sums")
    _check(out_ar.cpu().numpy(), reps * want_ar, reps * mass_ar, f"W={W} {reps} x {N_BIG} rows, AR log-likelihoods")
    small = kernels.two_sample(_dev(a), _dev(b), _dev(prior), HS, VANS, want_rows=True)[2]
    assert torch.equal(terms, small.repeat(reps, 1))                           # a row's term does not depend on where the row stands


def test_sixteen_models_in_one_call_and_seventeen_refused(base):
    """Sixteen models are four launches of four: each group has the bits of a call of its own, and the values of the SciPy twin."""
    _, a, b, prior = _table(base, 21, 300)
    hs, vans = 10.0 ** np.linspace(-3, 3, 7), 10.0 ** np.linspace(-2, 2, 9)
    ad, bd, pd = _dev(a), _dev(b), _dev(prior)
    out, _, terms = kernels.two_sample(ad, bd, pd, hs, vans, want_rows=True)
    assert out.shape == (16, 4) and terms.shape == (300, 16)
    for m0 in range(0, 16, 4):
        h4, v4 = hs[m0:m0 + 4], vans[max(m0 - 7, 0):max(m0 - 3, 0)]
        o4, _, t4 = kernels.two_sample(ad, bd, pd, h4 if h4.size else None, v4 if v4.size else None, want_rows=True)
        assert torch.equal(o4, out[m0:m0 + 4]) and torch.equal(t4, terms[:, m0:m0 + 4]), m0
    ok = a.astype(np.uint64).max(1) + b.astype(np.uint64).max(1) < 2 ** 31   # (float64 gammaln cancels at the counter's limit)
    sp, _ = tu.scipy_sums(a[ok], b[ok], prior[ok], hs, vans)
    got = kernels.two_sample(_dev(a[ok]), _dev(b[ok]), _dev(prior[ok]), hs, vans)[0].cpu().numpy()
    assert np.allclose(got, sp, rtol=1e-9, atol=1e-9 * np.abs(sp).max())
    with pytest.raises(ValueError, match=r"7 \+ 10 models"):
        kernels.two_sample(ad, bd, pd, hs, np.ones(10))                         # seventeen (the entry itself: tests/test_two_sample_cpu.py)
    with pytest.raises(ValueError, match="prior"):
        kernels.two_sample(ad, bd, None, hs, vans)


# ------------------------------------------------------------------------------------------- the stream contract
ENTRY = "bear_two_sample_f64"
STREAM_ARG = 10                  # the position of `void *stream` in the entry's declaration


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


def test_entry_keeps_the_stream_contract_on_a_side_stream(base, monkeypatch):
    """Class A of tests/test_stream_contract_gpu.py: conditions a-d of ``su.judge`` with a valid decoy table, and the handle in the
    entry's stream position is the side stream's."""
    from bear_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    _, a, b, prior = _table(base, 21, N_BIG)
    _, a2, b2, _ = _table(base, 21, N_BIG, seed=5)
    true = dict(a=_dev(a), b=_dev(b), f=_dev(prior))
    decoy = dict(a=_dev(b2), b=_dev(a2), f=torch.full_like(true["f"], 1.0 / 21))
    with torch.cuda.device(dev):
        h = su.Harness(dev)
        su.install_sentinel(monkeypatch)
        spy = _StreamSpy(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", spy)
        try:
            fails = su.judge(h, "two_sample", "A", true, decoy,
                             lambda i: kernels.two_sample(i["a"], i["b"], i["f"], HS, VANS, want_ar=True, want_rows=True), 1e-11, spy,
                             tol_from="the kernel's bound against mpmath")
        except RuntimeError as e:
            if any(s in str(e) for s in ("illegal memory access", "launch failure", "hipError 7")):
                pytest.exit(f"two_sample: the device faulted ({e}); nothing more is started on it", returncode=3)
            raise
    rec = h.records[-1]
    print(f"two_sample: gate {rec['gate_ms']:.1f} ms, host {rec['host_ms']:.3f} ms, device {rec['dev_ms']:.3f} ms, decoy gap "
          f"{rec['gap']:.3e}, side-stream distance {rec['dist']:.3e}")
    assert not fails, fails
    assert spy.streams and all(got == current for got, current in spy.streams), spy.streams
    assert h.side.cuda_stream != 0 and spy.streams[-1][0] == h.side.cuda_stream
    assert sum(1 for got, _ in spy.streams if got == h.side.cuda_stream) >= 2      # its first use there, and the judged call


# ------------------------------------------------------------------------------------------- the public calls
def _oracle_of_table(a, b, prior, hs, vans):
    """``oracle_sums`` and the per-row B_k and masses [N, M] of a whole table, paid per distinct row."""
    first, inverse = tu.unique_rows(a, b, prior)
    rows = tu.oracle_rows(a[first], b[first], prior[first], hs, vans)
    return tu.oracle_sums(rows, inverse), tu.as_float(rows[0][:, :, 3])[inverse], tu.as_float(rows[1][:, :, 3])[inverse]


def _check_result(res, oracle, n_h, what):
    (want, mass, want_ar, mass_ar), want_rows, mass_rows = oracle
    _check(res.log_bf, want[:, 3], mass[:, 3], what + " log_bf")
    _check(res.log_marg, want[:, :3], mass[:, :3], what + " log_marg")
    if res.log_ar is not None:
        _check(res.log_ar, want_ar, mass_ar, what + " log_ar")
        gof = res.gof_log_bf()
        assert gof.shape == (n_h, 2)
        _check(gof, want[:n_h, :2] - want_ar[None, :], mass[:n_h, :2] + mass_ar[None, :], what + " gof_log_bf")
    if res.per_kmer is not None:
        terms = res.per_kmer.cpu().numpy()
        _check(terms, want_rows, mass_rows, what + " per_kmer")
        _check(terms.sum(0), res.log_bf, mass[:, 3], what + " per_kmer summed", rtol=2 * RTOL)


def test_public_two_sample_on_the_bundled_table_in_pieces():
    hs, vans = np.array([0.05, 3.0]), np.array([1.0])
    data = dataloader.dataloader(YSD1, "dna", 501, 3)                          # pieces of 501 rows: the second starts off a 16-byte boundary
    assert data.num_rows > 2 * 501 and data.width == 5 and len(data.batch_bounds()) == 3
    ar_func, _ = ar_funcs.make_ar_func_linear(data.lag, 4, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    with torch.no_grad():
        prior = ar_func(torch.from_numpy(data.codes()).to("cuda")).to(torch.float64).cpu().numpy()
    a, b = data.counts[0], data.counts[1]
    oracle = _oracle_of_table(a, b, prior, hs, vans)
    res = hypothesis.two_sample(data, 0, 1, ar_func=ar_func, h=hs, vans=vans, per_kmer=True)
    assert res.models == ["bear(h=0.05)", "bear(h=3)", "van(1)"] and res.per_kmer.is_cuda and res.per_kmer.shape == (data.num_rows, 3)
    _check_result(res, oracle, 2, "ysd1 columns 0, 1 in 3 pieces")
    whole = hypothesis.two_sample(dataloader.dataloader(YSD1, "dna", 1 << 20, 3), 0, 1, ar_func=ar_func, h=hs, vans=vans)
    _check_result(whole, oracle, 2, "ysd1 columns 0, 1 in one piece")
    assert whole.per_kmer is None and np.abs(res.log_bf).min() > 1.0
    only_van = hypothesis.two_sample(data, 1, 0, vans=vans)                     # swapped columns, no AR function
    assert only_van.log_ar is None and only_van.gof_log_bf().shape == (0, 2) and only_van.models == ["van(1)"]
    _check(only_van.log_bf, oracle[0][0][2:, 3], oracle[0][1][2:, 3], "ysd1 columns 1, 0, vanilla")
    on_dev = dataloader.DeviceCountDataset(torch.from_numpy(data.kmers).to("cuda"), torch.from_numpy(data.counts.view(np.int32)).to("cuda"), "dna", 400)
    _check_result(hypothesis.two_sample(on_dev, 0, 1, ar_func=ar_func, h=hs, vans=vans, per_kmer=True), oracle, 2, "ysd1 as a device table")


@pytest.mark.parametrize("alphabet", ["dna", "prot"])
def test_public_two_sample_from_sequences(alphabet):
    """The statistical case of tests/test_two_sample_cpu.py counted and tested on the device: the values of the oracle on the
    device's own table, and the signs."""
    W = len(tu.LETTERS[alphabet]) + 1
    order, lags = tu.STAT_CASE[alphabet]
    P1, P2 = tu.chain(1, alphabet, order), tu.chain(2, alphabet, order)
    s10, s11, s12 = (tu.sample_seqs(P, s, alphabet, order=order) for P, s in ((P1, 10), (P1, 11), (P2, 12)))
    hs, vans = np.array([0.05, 5.0]), np.array([1.0])

    def uniform(codes):
        return torch.full((codes.shape[0], W), 1.0 / W, dtype=torch.float64, device=codes.device)
    for other, sign in ((s11, -1), (s12, +1)):
        results = hypothesis.two_sample_from_sequences(s10, other, lags, alphabet, ar_func=uniform, h=hs, vans=vans, per_kmer=True)
        text, group = summarize.encode_sequences(s10 + other, [0] * 100 + [1] * 100, False, alphabet)
        assert len(results) == len(lags)
        for lag, res in zip(lags, results):
            _, counts = summarize.count_transitions(text, group, lag, 2, alphabet=alphabet)
            a, b = np.ascontiguousarray(counts[0]), np.ascontiguousarray(counts[1])
            assert a.shape[1] == W and a.sum() == b.sum() == 100 * 121 and res.per_kmer.shape == (len(a), 3)
            _check_result(res, _oracle_of_table(a, b, np.full(a.shape, 1.0 / W), hs, vans), 2, f"{alphabet} lag {lag} sign {sign:+d}")
            print(f"{alphabet} lag {lag}: log BF {res.log_bf}")
            assert np.all(np.sign(res.log_bf) == sign), (alphabet, lag, sign, res.log_bf)
