"""GPU tests of the k-sample Bayes factors and the clustering of samples (kernels_ksample.h, kernels.k_sample, bear_amd.hypothesis):
the kernel against the formulas evaluated with mpmath at 50 digits (tests/k_sample_util.py) at both widths and 2, 3 and 16 groups,
against kernels.two_sample at two groups, its structure in equal bits, the grid stride, sixteen models, pooled counts at the
entry's limits, the deterministic library, the stream contract of include/bear_hip.h on a side stream (the entry's stream is not
its last parameter: same harness as tests/test_stream_contract_gpu.py, here) and the public calls.

The bound everywhere: ``|got - want| <= 1e-11 * mass``, ``mass`` the L1 sum of the lgamma brackets (resp. of the ``c log p`` terms)
behind that output -- for a bracket B the masses of all the T it is formed from; 2e-11 against kernels.two_sample, which sits within
1e-11 of the same oracle.  The largest ratio observed on an MI355X is printed per case and recorded in DESIGN.md 4.14."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import k_sample_util as ku
import stream_util as su
import two_sample_util as tu
from bear_amd import ar_funcs, dataloader, hypothesis, kernels, summarize
from conftest import ROOT, YSD1
from two_sample_util import HS, RTOL, VANS

pytestmark = pytest.mark.gpu

N_BIG = 4097
WIDTHS = (5, 21)


def _models(W, G):
    """Six models, but two (h = 0.7, van = 1) at width 21 with sixteen groups: the oracle is paid per T."""
    return (HS[1:2], VANS[1:2]) if (W, G) == (21, 16) else (HS, VANS)


def _dev(x):
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def _check(got, want, mass, what, rtol=RTOL):
    ratio = float((np.abs(got - want) / np.where(mass > 0, mass, 1.0)).max()) if got.size else 0.0
    print(f"k-sample {what}: largest |got - want| / mass = {ratio:.3e} (bound {rtol:.0e})")
    assert got.shape == want.shape and np.all(np.abs(got - want) <= rtol * mass), (what, ratio)


@pytest.fixture(scope="module")
def base():
    """(W, G) -> the G columns of rows of every kind, their prior rows, the models and the oracle, computed once when first asked for."""
    cache = {}

    def get(W, G):
        if (W, G) not in cache:
            cols, prior = ku.columns(W, G)
            hs, vans = _models(W, G)
            cache[W, G] = (cols, prior, hs, vans, ku.oracle_rows(cols, prior, hs, vans))
        return cache[W, G]
    return get


def _run(cols, prior, hs, vans, want_ar=True, want_rows=True, use=None):
    out = kernels.k_sample(_dev(cols), range(cols.shape[0]) if use is None else use, None if prior is None else _dev(prior), hs, vans,
                           want_ar=want_ar, want_rows=want_rows)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _check_all(got, rows, idx, what):
    """The five outputs of a call on the table ``base[idx]`` against the oracle; the row terms with exact zeros where at most one group
    has a transition -> the number of such rows."""
    out_group, out_pair, out_all, out_ar, terms = got
    want = ku.oracle_sums(rows, idx)
    for key, x in zip(ku.KEYS, (out_group, out_pair, out_all, out_ar)):
        _check(x, want[key][0], want[key][1], f"{what} {key} sums")
    _check(terms, tu.as_float(rows["all"][0][idx][:, :, 1]), tu.as_float(rows["all"][1][idx][:, :, 1]), f"{what} row terms")
    lone = np.array([all(v == 0 for v in r) for r in rows["all"][0][idx][:, :, 1]]) if len(idx) else np.zeros(0, bool)
    assert not terms[lone].view(np.int64).any()                                    # the bit pattern of +0.0
    return int(lone.sum())


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("size", ["1", "tile-1", "tile", "tile+1", "4097"])
def test_kernel_against_mpmath_at_sixteen_groups(base, W, size):
    tile = kernels.K_SAMPLE_TILE[W]
    assert tile == kernels.k_sample_tile(W, 16)
    n = {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "4097": N_BIG}[size]
    cols, prior, hs, vans, rows = base(W, 16)
    idx = tu.table_index(cols.shape[1], n)
    if n >= cols.shape[1]:
        assert set(idx.tolist()) == set(range(cols.shape[1]))                      # rows of every kind
    got = _run(cols[:, idx], prior[idx], hs, vans)
    assert got[0].shape == (len(hs) + len(vans), 16) and got[1].shape[1:] == (120, 2) and got[4].shape == (n, len(hs) + len(vans))
    _check_all(got, rows, idx, f"W={W} G=16 n={n}")
    assert not got[0][:, -1].view(np.int64).any()                                  # the all-zero column: exactly +0.0 ...
    assert not got[1][:, [p for p, (g, g2) in enumerate(ku.pairs(16)) if g2 == 15], 1].view(np.int64).any()     # ... in every B it takes part in
    if n > 1:
        assert np.abs(got[0][:, :-1]).min() > 0 and np.abs(got[2]).min() > 0
    again = _run(cols[:, idx], prior[idx], hs, vans)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))             # the same call twice: equal bits


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("G", [2, 3])
def test_kernel_against_mpmath_at_two_and_three_groups(base, W, G):
    cols, prior, hs, vans, rows = base(W, G)
    idx = tu.table_index(cols.shape[1], N_BIG)
    got = _run(cols[:, idx], prior[idx], hs, vans)
    lone = _check_all(got, rows, idx, f"W={W} G={G} n={N_BIG}")
    assert lone > 0 and np.abs(got[4]).max() > 0                                    # rows of one group, or of none, are there


@pytest.mark.parametrize("W", WIDTHS)
def test_two_groups_against_two_sample(base, W):
    """The same pair through ``kernels.two_sample``: both within 1e-11 of the mass from the oracle, so 2e-11 apart."""
    cols, prior, hs, vans, rows = base(W, 2)
    idx = tu.table_index(cols.shape[1], N_BIG, seed=2)
    mass = ku.oracle_sums(rows, idx)
    out_group, out_pair, out_all, out_ar, terms = _run(cols[:, idx], prior[idx], hs, vans)
    ts, ts_ar, ts_terms = (t.cpu().numpy() for t in kernels.two_sample(_dev(cols[0, idx]), _dev(cols[1, idx]), _dev(prior[idx]), hs, vans,
                                                                       want_ar=True, want_rows=True))
    _check(out_group, ts[:, :2], mass["group"][1], f"W={W} M_a, M_b against two_sample", rtol=2 * RTOL)
    _check(out_pair[:, 0], ts[:, 2:], mass["pair"][1][:, 0], f"W={W} M_ab, B against two_sample", rtol=2 * RTOL)
    _check(out_all, ts[:, 2:], mass["all"][1], f"W={W} all groups against two_sample", rtol=2 * RTOL)
    _check(out_ar, ts_ar, mass["ar"][1], f"W={W} L_a, L_b against two_sample", rtol=2 * RTOL)
    _check(terms, ts_terms, tu.as_float(rows["all"][1][idx][:, :, 1]), f"W={W} row terms against two_sample", rtol=2 * RTOL)


@pytest.mark.parametrize("W", WIDTHS)
def test_structure_in_equal_bits(base, W):
    cols, prior, hs, vans, rows = base(W, 16)
    idx = tu.table_index(cols.shape[1], N_BIG, seed=1)
    c, f = cols[:, idx], prior[idx]
    M = len(hs) + len(vans)
    full = _run(c, f, hs, vans)
    # in place (columns of 4096 rows start on 16-byte boundaries) and copied (the same rows of the 4097-row table do not): equal bits
    cd, fd = _dev(c), _dev(f)
    assert (cd.data_ptr() + 4 * cd.stride(0)) % 16 and not (cd[:, :4096].contiguous().stride(0) * 4) % 16
    placed = kernels.k_sample(cd[:, :4096].contiguous(), range(16), fd[:4096], hs, vans, want_ar=True, want_rows=True)
    copied = kernels.k_sample(cd[:, :4096], range(16), fd[:4096], hs, vans, want_ar=True, want_rows=True)
    assert all(torch.equal(x, y) for x, y in zip(placed, copied))
    for want_ar, want_rows in ((False, True), (True, False), (False, False)):      # omitted outputs do not change the others
        got = _run(c, f, hs, vans, want_ar=want_ar, want_rows=want_rows)
        assert (got[3] is None) != want_ar and (got[4] is None) != want_rows
        assert all(x is None or x.tobytes() == y.tobytes() for x, y in zip(got, full))
    van = _run(c, None, None, vans, want_ar=False)                                  # vanilla models alone, no prior rows
    for x, y in zip(van[:3] + van[4:], full[:3] + full[4:]):
        assert x.tobytes() == np.ascontiguousarray(y[len(hs):] if y.shape[0] == M else y[:, len(hs):]).tobytes()
    zero = _run(c[:, :0], f[:0], hs, vans)                                          # no rows: zeros
    assert zero[0].shape == (M, 16) and zero[1].shape == (M, 120, 2) and zero[4].shape == (0, M)
    assert not any(x.any() for x in zero)
    # a subset of the columns in another order: the oracle's groups and pairs of that order (other bits than the full call's)
    use, want = [5, 0, 14, 3], ku.oracle_sums(rows, idx)
    sub = tuple(None if t is None else t.cpu().numpy() for t in kernels.k_sample(cd, use, fd, hs, vans, want_ar=True))
    where = {pair: p for p, pair in enumerate(ku.pairs(16))}
    at = [where[tuple(sorted((use[g], use[g2])))] for g, g2 in ku.pairs(4)]
    _check(sub[0], want["group"][0][:, use], want["group"][1][:, use], f"W={W} columns {use} group sums")
    _check(sub[1], want["pair"][0][:, at], want["pair"][1][:, at], f"W={W} columns {use} pair sums")
    _check(sub[3], want["ar"][0][use], want["ar"][1][use], f"W={W} columns {use} AR sums")


def test_pooled_counts_at_the_limits():
    """Every cell of all sixteen columns at 0xFFFFFFFF: a pooled cell of 2^36 - 16, a row total above 2^40 -- exact integers."""
    for W in WIDTHS:
        cols, prior = ku.limit_rows(W)
        assert int(cols.astype(np.uint64).sum(0).max()) == 2 ** 36 - 16 and (W == 5 or cols.astype(np.uint64).sum((0, 2)).max() > 2 ** 40)
        rows = ku.oracle_rows(cols, prior, HS[1:2], VANS[1:2])
        _check_all(_run(cols, prior, HS[1:2], VANS[1:2]), rows, np.arange(3), f"W={W} G=16 at the limits")


@pytest.mark.parametrize("W", WIDTHS)
def test_grid_stride(base, W):
    """More tiles than a launch has blocks (blocks per CU x 256 CUs): the 4097-row table repeated sums to the repeat count times its
    oracle, and a row's term does not depend on where the row stands."""
    cols, prior, hs, vans, rows = base(W, 16)
    idx = tu.table_index(cols.shape[1], N_BIG)
    tile = kernels.K_SAMPLE_TILE[W]
    reps = kernels.K_SAMPLE_BLOCKS_PER_CU * 256 * tile // N_BIG + 2
    assert reps * N_BIG > kernels.K_SAMPLE_BLOCKS_PER_CU * 256 * tile + tile
    cd, fd = _dev(cols[:, idx]), _dev(prior[idx])
    got = kernels.k_sample(cd.repeat(1, reps, 1), range(16), fd.repeat(reps, 1), hs, vans, want_ar=True, want_rows=True)
    want = ku.oracle_sums(rows, idx)
    for key, x in zip(ku.KEYS, got[:4]):
        _check(x.cpu().numpy(), reps * want[key][0], reps * want[key][1], f"W={W} {reps} x {N_BIG} rows, {key} sums")
    small = kernels.k_sample(cd, range(16), fd, hs, vans, want_rows=True)[4]
    assert torch.equal(got[4], small.repeat(reps, 1))


def test_sixteen_models_in_one_call_and_seventeen_refused(base):
    """Sixteen models are four launches of four: each group has the bits of a call of its own, and the values of the SciPy twin."""
    cols, prior = base(21, 3)[:2]
    idx = tu.table_index(cols.shape[1], 300)
    c, f = cols[:, idx], prior[idx]
    hs, vans = 10.0 ** np.linspace(-3, 3, 7), 10.0 ** np.linspace(-2, 2, 9)
    cd, fd = _dev(c), _dev(f)
    full = kernels.k_sample(cd, range(3), fd, hs, vans, want_rows=True)
    assert full[0].shape == (16, 3) and full[1].shape == (16, 3, 2) and full[2].shape == (16, 2) and full[4].shape == (300, 16)
    for m0 in range(0, 16, 4):
        h4, v4 = hs[m0:m0 + 4], vans[max(m0 - 7, 0):max(m0 - 3, 0)]
        part = kernels.k_sample(cd, range(3), fd, h4 if h4.size else None, v4 if v4.size else None, want_rows=True)
        assert all(torch.equal(part[k], full[k][m0:m0 + 4]) for k in range(3)) and torch.equal(part[4], full[4][:, m0:m0 + 4]), m0
    ok = c.astype(np.uint64).max((0, 2)) < 2 ** 31 // 3                            # (float64 gammaln cancels at the counter's limit)
    twin = ku.scipy_sums(c[:, ok], f[ok], hs, vans)
    got = kernels.k_sample(_dev(c[:, ok]), range(3), _dev(f[ok]), hs, vans)
    for x, y in zip(got[:3], twin[:3]):
        assert np.allclose(x.cpu().numpy(), y, rtol=1e-9, atol=1e-9 * np.abs(y).max())
    with pytest.raises(ValueError, match=r"7 \+ 10 models"):
        kernels.k_sample(cd, range(3), fd, hs, np.ones(10))                         # seventeen (the entry itself: tests/test_k_sample_cpu.py)
    with pytest.raises(ValueError, match="prior"):
        kernels.k_sample(cd, range(3), None, hs, vans)
    with pytest.raises(ValueError, match="columns"):
        kernels.k_sample(cd, [0], fd, hs, vans)
    with pytest.raises(ValueError, match="the table has 3"):
        kernels.k_sample(cd, [0, 3], fd, hs, vans)


_DET_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from bear_amd import _lib
import test_k_sample_gpu as t
import k_sample_util as ku
import two_sample_util as tu
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
cols, prior = ku.columns(21, 16)
idx = tu.table_index(cols.shape[1], t.N_BIG, 1)
got = t._run(cols[:, idx], prior[idx], *t._models(21, 16))
np.savez(sys.argv[2], **{"out%d" % k: x for k, x in enumerate(got)})
"""


def test_deterministic_library_returns_the_same_bits(base, tmp_path):
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 0 or os.environ.get("BEAR_AMD_DETERMINISTIC")
    cols, prior, hs, vans, _ = base(21, 16)
    idx = tu.table_index(cols.shape[1], N_BIG, 1)
    here = _run(cols[:, idx], prior[idx], hs, vans)
    script = tmp_path / "det_k_sample.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "det.npz")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    there = np.load(tmp_path / "det.npz")
    for k, x in enumerate(here):
        assert there["out%d" % k].shape == x.shape and there["out%d" % k].tobytes() == x.tobytes(), k


# ------------------------------------------------------------------------------------------- the stream contract
ENTRY = "bear_k_sample_f64"
STREAM_ARG = 11                  # the position of `void *stream` in the entry's declaration


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
    cols, prior, hs, vans, _ = base(21, 16)
    idx, idx2 = tu.table_index(cols.shape[1], 4096), tu.table_index(cols.shape[1], 4096, seed=5)      # 4096 rows: the table is used in place
    true = dict(c=_dev(cols[:, idx]), f=_dev(prior[idx]))
    decoy = dict(c=_dev(cols[::-1, idx2]), f=torch.full_like(true["f"], 1.0 / 21))
    with torch.cuda.device(dev):
        h = su.Harness(dev)
        # As in tests/test_classify_gpu.py: torch hands out its pooled streams in turn and the runtime deals them over its few
        # hardware queues in turn, so a harness that takes two streams moves every later side stream of the session onto another
        # queue -- with this test's two alone, the first case of tests/test_stream_contract_gpu.py landed on the null stream's queue,
        # ran behind the null gate and missed condition d.  Two more make four: later tests get the queues they have without this one.
        spare = [torch.cuda.Stream(dev) for _ in range(2)]
        assert len({s.cuda_stream for s in spare} | {h.side.cuda_stream, h.side2.cuda_stream}) == 4
        su.install_sentinel(monkeypatch)
        spy = _StreamSpy(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", spy)
        try:
            fails = su.judge(h, "k_sample", "A", true, decoy,
                             lambda i: kernels.k_sample(i["c"], range(16), i["f"], hs, vans, want_ar=True, want_rows=True), 1e-11, spy,
                             tol_from="the kernel's bound against mpmath")
        except RuntimeError as e:
            if any(s in str(e) for s in ("illegal memory access", "launch failure", "hipError 7")):
                pytest.exit(f"k_sample: the device faulted ({e}); nothing more is started on it", returncode=3)
            raise
    rec = h.records[-1]
    print(f"k_sample: gate {rec['gate_ms']:.1f} ms, host {rec['host_ms']:.3f} ms, device {rec['dev_ms']:.3f} ms, decoy gap "
          f"{rec['gap']:.3e}, side-stream distance {rec['dist']:.3e}")
    assert not fails, fails
    assert spy.streams and all(got == current for got, current in spy.streams), spy.streams
    assert h.side.cuda_stream != 0 and spy.streams[-1][0] == h.side.cuda_stream
    assert sum(1 for got, _ in spy.streams if got == h.side.cuda_stream) >= 2      # its first use there, and the judged call


# ------------------------------------------------------------------------------------------- the public calls
def _oracle_of_table(cols, prior, hs, vans):
    """``ku.oracle_sums`` and the per-row all-groups bracket and its mass [N, M] of a whole table, paid per distinct row."""
    first, inverse = ku.unique_rows(cols, prior)
    rows = ku.oracle_rows(cols[:, first], prior[first], hs, vans)
    return ku.oracle_sums(rows, inverse), tu.as_float(rows["all"][0][:, :, 1])[inverse], tu.as_float(rows["all"][1][:, :, 1])[inverse]


def _check_result(res, oracle, n_h, what):
    sums, want_rows, mass_rows = oracle
    G = res.log_marg.shape[1]
    _check(res.log_marg, *sums["group"], what + " log_marg")
    _check(res.log_marg_all, sums["all"][0][:, 0], sums["all"][1][:, 0], what + " log_marg_all")
    _check(res.log_bf_all, sums["all"][0][:, 1], sums["all"][1][:, 1], what + " log_bf_all")
    for p, (g, g2) in enumerate(ku.pairs(G)):
        for name, k in (("log_marg_pair", 0), ("log_bf", 1)):
            full = getattr(res, name)
            assert np.array_equal(full[:, g, g2], full[:, g2, g])
            _check(full[:, g, g2], sums["pair"][0][:, p, k], sums["pair"][1][:, p, k], f"{what} {name} ({g}, {g2})")
    for m in range(res.log_bf.shape[0]):
        assert not np.diag(res.log_bf[m]).view(np.int64).any() and np.array_equal(np.diag(res.log_marg_pair[m]), res.log_marg[m])
    if res.log_ar is not None:
        _check(res.log_ar, *sums["ar"], what + " log_ar")
        gof = res.gof_log_bf()
        assert gof.shape == (n_h, G)
        _check(gof, sums["group"][0][:n_h] - sums["ar"][0][None, :], sums["group"][1][:n_h] + sums["ar"][1][None, :], what + " gof_log_bf")
    if res.per_kmer is not None:
        terms = res.per_kmer.cpu().numpy()
        _check(terms, want_rows, mass_rows, what + " per_kmer")
        _check(terms.sum(0), res.log_bf_all, sums["all"][1][:, 1], what + " per_kmer summed", rtol=2 * RTOL)


def test_public_k_sample_on_the_bundled_table():
    hs, vans = np.array([0.05, 3.0]), np.array([1.0])
    data = dataloader.dataloader(YSD1, "dna", 501, 3)                          # pieces of 501 rows: the second starts off a 16-byte boundary
    assert data.num_rows > 2 * 501 and data.width == 5 and data.num_ds == 3 and len(data.batch_bounds()) == 3
    ar_func, _ = ar_funcs.make_ar_func_linear(data.lag, 4, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    with torch.no_grad():
        prior = ar_func(torch.from_numpy(data.codes()).to("cuda")).to(torch.float64).cpu().numpy()
    oracle = _oracle_of_table(data.counts, prior, hs, vans)
    res = hypothesis.k_sample(data, ar_func=ar_func, h=hs, vans=vans, per_kmer=True)
    assert res.models == ["bear(h=0.05)", "bear(h=3)", "van(1)"] and res.per_kmer.is_cuda and res.per_kmer.shape == (data.num_rows, 3)
    _check_result(res, oracle, 2, "ysd1 in 3 pieces")
    whole = hypothesis.k_sample(dataloader.dataloader(YSD1, "dna", 1 << 20, 3), [0, 1, 2], ar_func=ar_func, h=hs, vans=vans)
    _check_result(whole, oracle, 2, "ysd1 in one piece")
    assert whole.per_kmer is None and np.abs(res.log_bf[:, 0, 1]).min() > 1.0
    on_dev = dataloader.DeviceCountDataset(torch.from_numpy(data.kmers).to("cuda"), torch.from_numpy(data.counts.view(np.int32)).to("cuda"), "dna", 400)
    _check_result(hypothesis.k_sample(on_dev, ar_func=ar_func, h=hs, vans=vans, per_kmer=True), oracle, 2, "ysd1 as a device table")
    # a subset in another order, from the host table and in place from the device table; vanilla alone
    sub_oracle = _oracle_of_table(data.counts[[2, 0]], prior, hs[:0], vans)
    for table, what in ((data, "host"), (on_dev, "device")):
        sub = hypothesis.k_sample(table, cols=(2, 0), vans=vans, per_kmer=True)
        assert sub.log_ar is None and sub.gof_log_bf().shape == (0, 2) and sub.models == ["van(1)"] and sub.log_bf.shape == (1, 2, 2)
        _check_result(sub, sub_oracle, 0, f"ysd1 columns 2, 0 of the {what} table, vanilla")
    two = hypothesis.two_sample(data, 2, 0, vans=vans)
    _check(sub.log_bf[:, 0, 1], two.log_bf, sub_oracle[0]["pair"][1][:, 0, 1], "ysd1 columns 2, 0 against two_sample", rtol=2 * RTOL)


@pytest.mark.parametrize("alphabet", ["dna", "prot"])
def test_from_sequences_and_agglomerate_on_the_statistical_case(alphabet):
    """The six-group case of tests/test_k_sample_cpu.py counted, tested and clustered on the device: the values of the oracle on the
    device's own table, the pair signs, the partition, and evidence steps of -log_bf."""
    W = len(tu.LETTERS[alphabet]) + 1
    lags = tu.STAT_CASE[alphabet][1]
    seqs = ku.stat_sequences(alphabet)
    hs, vans = ku.STAT_HS, ku.STAT_VANS

    def uniform(codes):
        return torch.full((codes.shape[0], W), 1.0 / W, dtype=torch.float64, device=codes.device)
    results = hypothesis.k_sample_from_sequences(seqs, lags, alphabet, ar_func=uniform, h=hs, vans=vans, per_kmer=True)
    text, group = summarize.encode_sequences([s for g in seqs for s in g], [g for g in range(6) for _ in range(100)], False, alphabet)
    assert len(results) == len(lags)
    same = [(g, g2) for g, g2 in ku.pairs(6) if (g - g2) % 2 == 0]
    for lag, res in zip(lags, results):
        kmers, counts = summarize.count_transitions(text, group, lag, 6, alphabet=alphabet)
        assert counts.shape[0] == 6 and counts.shape[2] == W and np.all(counts.sum((1, 2)) == 100 * 121)
        assert res.per_kmer.shape == (counts.shape[1], 3) and res.log_bf.shape == (3, 6, 6)
        oracle = _oracle_of_table(np.ascontiguousarray(counts), np.full(counts.shape[1:], 1.0 / W), hs, vans)
        _check_result(res, oracle, 2, f"{alphabet} lag {lag}")
        print(f"{alphabet} lag {lag}: same source max {max(res.log_bf[:, g, g2].max() for g, g2 in same):.1f}, cross min "
              f"{min(res.log_bf[:, g, g2].min() for g, g2 in ku.pairs(6) if (g, g2) not in same):.1f}, all six {res.log_bf_all}")
        for g, g2 in ku.pairs(6):
            assert np.all(res.log_bf[:, g, g2] <= -46) if (g, g2) in same else np.all(res.log_bf[:, g, g2] >= 147), (lag, g, g2)
        data = dataloader.DeviceCountDataset(torch.from_numpy(kmers).to("cuda"), torch.from_numpy(np.ascontiguousarray(counts).view(np.int32)).to("cuda"),
                                             alphabet, 1 << 30)
        for m in range(3):
            agg = hypothesis.agglomerate(data, model=m, ar_func=uniform, h=hs, vans=vans)
            assert agg.partition == ku.PARTITION and len(agg.merges) == 4 and agg.log_evidence.shape == (5,)
            # a step's gain is -log_bf of its merge.  Behind the gain: the evidence before and after (every cluster's T), behind log_bf
            # the two clusters' and their pooled T.  The mass of T grows faster than the counts, so each of the four -- evidence
            # before, evidence after, the two clusters, the pooled cluster -- is below the mass of the all-groups bracket (every
            # group's T and the T of all six pooled): 4 x 1e-11 of that mass.
            mass = oracle[0]["all"][1][m, 1]
            assert np.all(np.abs(np.diff(agg.log_evidence) + [x for _, _, x in agg.merges]) <= 4 * RTOL * mass), (lag, m)
            assert all(x <= -46 for _, _, x in agg.merges)
        p1 = hypothesis.k_sample(data, cols=(0, 2, 4), ar_func=uniform, h=hs, vans=vans)
        assert np.all(p1.log_bf_all <= -99)
        host = dataloader.CountDataset(kmers, np.ascontiguousarray(counts), alphabet, 1 << 30)
        assert hypothesis.agglomerate(host, cols=(5, 0, 3, 2), vans=vans).partition == [[0, 2], [3, 5]]
