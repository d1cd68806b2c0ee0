"""The width-generic kernels (kernels_wide.h: dm_wide_kernel, eval_wide_kernel) at the sizes and edges where such code goes wrong:
edge rows and priors over the h grid, extreme h against mpmath, tables large enough that every block strides over several tiles,
the W = 5 twin against the trusted 5-wide entry points, sharding, reproducibility, graph replay with h updated in place, and the
evaluation against the NumPy oracle.  Mode N is held to the width-generic C oracle (c_oracle.dm_prior_w, every item in long double)
with the tolerances of test_parity_gpu.py: sum LL 1e-11 relative, d/dh_signed 2e-13 of its L1 mass, every gradient-row entry
1e-12 of its own mass (AR mode: 1e-12 relative)."""
import numpy as np
import pytest
import torch

import bear_oracle as o
import c_oracle as co
from bear_amd import kernels
from test_parity_gpu import CASES_REF
from test_prot_cpu import make_prot_table
from test_prot_gpu import HashNoiseW
from util import PRIOR_KINDS, edge_table_wide, prior_rows, prior_rows_wide, sparse_table, tile_rows, wide_scale_table

pytestmark = pytest.mark.gpu
EPS = 1e-7
NTH = 16                       # oracle threads
ELBO_RTOL, MASS_RTOL, ROW_RTOL = 1e-11, 2e-13, 1e-12
# sum LL may cancel far below the terms it is the sum of: the row [2^32 - 1, 0, ..., 0] alone has items of ~9.1e10 (L1 mass 1.8e11,
# one double ulp there 1.5e-5) that leave an LL of -6242 .. -3e-5.  No fp64 evaluation gets such a sum to 1e-11 of itself; it is
# held to 1e-11 of itself PLUS 1e-15 of its L1 mass (c_oracle.dm_prior_mass_w: |row term| + sum |items|, the scale of its
# rounding).  Observed on such rows: 1e-17 .. 7e-17 of the mass.
COND_RTOL = 1e-15
# kernels_wide.h / bear_eval.hip: rows per tile of dm_wide_kernel, its blocks per CU; eval_wide_kernel's rows per tile, blocks per CU
WIDE_TILE = {21: 128, 5: 512}
WIDE_BLOCKS_PER_CU, EVW_ROWS, EVAL_BLOCKS_PER_CU = 4, 128, 8


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dc(c):
    return torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda()


def _df(f):
    return torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).cuda()


def _hdev(h_s):
    return torch.tensor([h_s], dtype=torch.float64, device="cuda")


def _run(c, f, h_s, train_ar, want_grad):
    out, g = kernels.dm_prior_wide(_dc(c), _df(f), _hdev(h_s), train_ar=train_ar, want_grad=want_grad)
    return out.cpu().numpy(), (g.cpu().numpy() if g is not None else None)


def _errors(got, g, c, f, h_s, train_ar, want_grad, what):
    """The oracle's verdict on one kernel call: a list of (what, error / allowed) for every quantity past its tolerance."""
    want, wg = co.dm_prior_w(c, f, h_s, train_ar=train_ar, want_grad=want_grad, nthreads=NTH)
    mass, gm = co.dm_prior_mass_w(c, f, h_s, train_ar=train_ar, want_grad=want_grad, nthreads=NTH)
    bad = []
    r = abs(got[0] - want[0]) / max(ELBO_RTOL * abs(want[0]) + COND_RTOL * mass[1], 1e-300)
    if r > 1 or not np.isfinite(got[0]):
        bad.append((what, "ll", got[0], want[0], mass[1], r))
    if train_ar:
        if got[1] != 0.0:
            bad.append((what, "dh", got[1], 0.0, np.inf))
    else:
        r = abs(got[1] - want[1]) / (MASS_RTOL * mass[0] + 1e-14)
        if r > 1 or not np.isfinite(got[1]):
            bad.append((what, "dh", got[1], want[1], r))
    if want_grad:
        allowed = ROW_RTOL * (np.abs(wg) if train_ar else gm)
        err = np.abs(g - wg)
        over = ~(err <= allowed)                   # an exact 0 allowed: only an exact match passes (NaN fails)
        if over.any():
            i = np.unravel_index(np.argmax(np.where(over, err / np.maximum(allowed, 1e-300), 0)), g.shape)
            bad.append((what, "grad", i, g[i], wg[i], allowed[i], int(over.sum())))
    return bad


# ------------------------------------------------------------------ edge rows, W = 21
H_EDGE = (-6.0, -3.0, 0.0, 0.37, 2.5, 6.0)
N_EDGE = (1, 127, 128, 129, 1037)


@pytest.mark.parametrize("want_grad", [False, True])
@pytest.mark.parametrize("train_ar", [False, True])
@pytest.mark.parametrize("kind", PRIOR_KINDS)
def test_edge_rows_w21(kind, train_ar, want_grad):
    table = edge_table_wide(21)
    bad = []
    for n in N_EDGE:
        c = tile_rows(table, n, seed=n)
        f = prior_rows_wide(n, 21, kind, seed=n)
        for h_s in (H_EDGE if not train_ar else (0.37,)):
            got, g = _run(c, f, h_s, train_ar, want_grad)
            if want_grad:
                assert g.shape == c.shape and (g[c.sum(1) == 0] == 0).all()
            else:
                assert g is None
            bad += _errors(got, g, c, f, h_s, train_ar, want_grad, (n, h_s))
    assert not bad, "\n".join(map(str, bad))


H_LARGE = (-30.0, -45.0)   # concentrations up to 21 e^45 = 7e20: past the 2^60 switch of the item routine (the oracle's items are held
#                            to mpmath there: test_oracle.py::test_oracle_w_items_match_mpmath)


@pytest.mark.parametrize("want_grad", [False, True])
@pytest.mark.parametrize("kind", ["softmax", "tiny"])
def test_edge_rows_w21_large_concentrations(kind, want_grad):
    c = edge_table_wide(21)
    f = prior_rows_wide(len(c), 21, kind, seed=11)
    bad = []
    for h_s in H_LARGE:
        got, g = _run(c, f, h_s, False, want_grad)
        bad += _errors(got, g, c, f, h_s, False, want_grad, h_s)
    assert not bad, "\n".join(map(str, bad))


def _mp_rows(c, f, h_s, eps=EPS):
    """sum LL, d/dh_signed, gradient rows and their masses at 40 digits (mpmath)."""
    import mpmath as mp
    mp.mp.dps = 40
    h = mp.exp(mp.mpf(h_s))
    ll = dh = mll = mdh = mp.mpf(0)
    g = np.zeros(c.shape)
    gm = np.zeros(c.shape)
    for i in range(len(c)):
        a = [mp.mpf(float(x)) / h + mp.mpf(eps) for x in f[i]]
        n = mp.mpf(int(c[i].sum(dtype=np.uint64)))
        A = mp.fsum(a)
        if n == 0:
            continue
        Dn, Pn = mp.loggamma(A + n) - mp.loggamma(A), mp.digamma(A + n) - mp.digamma(A)
        ll -= Dn
        mll += abs(Dn)
        for b in range(c.shape[1]):
            cb = mp.mpf(int(c[i, b]))
            Db, Pb = (mp.loggamma(a[b] + cb) - mp.loggamma(a[b]), mp.digamma(a[b] + cb) - mp.digamma(a[b])) if cb else (0, 0)
            ll += Db
            mll += abs(Db)
            fb = mp.mpf(float(f[i, b]))
            dh -= (Pb - Pn) * fb / h
            mdh += (abs(Pb) + abs(Pn)) * fb / h
            g[i, b] = float((Pb - Pn) / h)
            gm[i, b] = float((abs(Pb) + abs(Pn)) / h)
    return float(ll), float(dh), g, float(mll), float(mdh), gm


@pytest.mark.parametrize("h_s", [-20.0, 10.0])
def test_extreme_h_matches_mpmath(h_s):
    """h_signed = -20 puts concentrations of ~1e9 against counts of 1 .. 2^32 - 1, h_signed = 10 all of them near eps."""
    pytest.importorskip("mpmath")
    table = edge_table_wide(21)
    c = tile_rows(table, 101, seed=3)
    f = np.concatenate([prior_rows_wide(26, 21, k, seed=5) for k in PRIOR_KINDS])[:101]
    got, g = _run(c, f, h_s, False, True)
    ll, dh, wg, mll, mdh, gm = _mp_rows(c, f, h_s)
    assert abs(got[0] - ll) <= ELBO_RTOL * abs(ll) + COND_RTOL * mll, (got[0], ll, mll)
    assert abs(got[1] - dh) <= MASS_RTOL * mdh + 1e-14, (got[1], dh, mdh)
    err = np.abs(g - wg)
    assert (err <= ROW_RTOL * gm).all(), np.max(err / np.maximum(gm, 1e-300))
    # and the C oracle the other tests lean on, at the same point
    want, wgo = co.dm_prior_w(c, f, h_s, want_grad=True)
    assert abs(want[0] - ll) <= 1e-14 * mll and abs(want[1] - dh) <= 1e-14 * mdh and (np.abs(wgo - wg) <= 1e-14 * gm).all()


# ------------------------------------------------------------------ grid-stride scale
SCALE = [(21, 300_003, False, 2), (21, 300_003, True, 2), (21, 1_330_003, False, 10), (21, 1_330_003, True, 10),
         (5, 1_100_001, False, 2)]


@pytest.mark.parametrize("W,n,dense,min_tiles", SCALE, ids=[f"W{w}-{n}-{'dense' if d else 'sparse'}" for w, n, d, _ in SCALE])
def test_grid_stride_scale(W, n, dense, min_tiles):
    assert n % 4 and n % WIDE_TILE[W]
    grid = _cu() * WIDE_BLOCKS_PER_CU
    tiles = -(-n // WIDE_TILE[W])
    assert tiles // grid >= min_tiles, (tiles, grid)          # every block runs the tile loop at least min_tiles times
    c = wide_scale_table(n, W, dense=dense, seed=n + W)
    f = prior_rows_wide(n, W, "tiny" if not dense else "scaled", seed=W)
    cd, fd, hd = _dc(c), _df(f), _hdev(-0.6)
    bad = []
    for train_ar in (False, True):
        out, g = kernels.dm_prior_wide(cd, fd, hd, train_ar=train_ar, want_grad=True)
        got, g = out.cpu().numpy(), g.cpu().numpy()
        out2, _ = kernels.dm_prior_wide(cd, fd, hd, train_ar=train_ar, want_grad=False)
        assert np.array_equal(out2.cpu().numpy(), got)           # GRAD changes what is written, not the sums
        bad += _errors(got, g, c, f, -0.6, train_ar, True, ("ar" if train_ar else "bear", n))
        del g
    assert not bad, bad


# ------------------------------------------------------------------ the W = 5 twin against the trusted 5-wide kernels
def _twin_check(cd, fd, h_s, train_ar, want_grad, mass_h, gmass):
    ref, gref = kernels.dm_prior(cd, fd, h_s, train_ar=train_ar, want_grad=want_grad)
    got, g = kernels.dm_prior_wide(cd, fd, _hdev(h_s), train_ar=train_ar, want_grad=want_grad)
    ref, got = ref.cpu().numpy(), got.cpu().numpy()
    assert abs(got[0] - ref[0]) <= 1e-12 * abs(ref[0]), (got, ref)
    assert abs(got[1] - ref[1]) <= (0.0 if train_ar else MASS_RTOL * mass_h + 1e-14), (got, ref, mass_h)
    if want_grad:
        allowed = ROW_RTOL * (gref.abs() if train_ar else gmass)
        assert bool(((g - gref).abs() <= allowed).all()), float(((g - gref).abs() - allowed).max())


@pytest.mark.parametrize("case", list(CASES_REF))
def test_w5_twin_matches_5_wide_kernels(case, ysd1):
    c = ysd1[1][:, 0].astype(np.uint32) if case == "ysd1" else CASES_REF[case]()[0]
    f = prior_rows(len(c), 6)
    cd, fd = _dc(c), _df(f)
    for h_s in (-3.0, -0.4, 2.5):
        for train_ar in (False, True):
            mass, gm = co.dm_prior_mass_w(c, f, h_s, train_ar=train_ar, want_grad=True, nthreads=NTH)
            for want_grad in (False, True):
                _twin_check(cd, fd, h_s, train_ar, want_grad, mass[0], _df(gm))


def _torch_masses(cd, fd, h_s):
    """L1 masses of d/dh_signed and of each gradient-row entry, on the device (torch.digamma: a tolerance scale only)."""
    h = float(np.exp(h_s))
    c = cd.view(torch.int32).to(torch.float64)
    c = torch.where(c < 0, c + 2.0 ** 32, c)
    a = fd / h + EPS
    A, n = a.sum(1, keepdim=True), c.sum(1, keepdim=True)
    pn = (torch.digamma(A + n) - torch.digamma(A)).abs()
    pb = (torch.digamma(a + c) - torch.digamma(a)).abs()
    gm = (pb + pn) / h
    return float((gm * fd.abs()).sum()), gm


def test_w5_twin_matches_5_wide_kernels_2e7():
    n = 20_000_000
    dev = torch.device("cuda", 0)
    cd = kernels.synth_counts(21, 0, n, dev, want=("train",))["train"]
    fd = kernels.synth_prior(21, 0, n, dev)
    for h_s in (-3.0, -0.4, 2.5):
        mass_h, gm = _torch_masses(cd, fd, h_s)
        for train_ar in (False, True):
            for want_grad in (False, True):
                _twin_check(cd, fd, h_s, train_ar, want_grad, mass_h, gm)
        del gm


# ------------------------------------------------------------------ sharding, reproducibility, graph replay
@pytest.fixture(scope="module")
def mid_table():
    n = 300_003
    return wide_scale_table(n, 21, seed=41), prior_rows_wide(n, 21, "tiny", seed=41)


@pytest.mark.parametrize("train_ar", [False, True])
def test_sharded_sum_equals_whole(train_ar, mid_table):
    c, f = mid_table
    n = len(c)
    cd, fd, hd = _dc(c), _df(f), _hdev(0.37)
    whole, gw = kernels.dm_prior_wide(cd, fd, hd, train_ar=train_ar, want_grad=True)
    whole = whole.cpu().numpy()
    cuts = [0, 1, 1023, 5001, 77_777, 200_002, n]              # starts 1, 1023, 5001, 77777: not multiples of 4 (the clone path)
    acc = np.zeros(2)
    for a, b in zip(cuts[:-1], cuts[1:]):
        out, g = kernels.dm_prior_wide(cd[a:b], fd[a:b], hd, train_ar=train_ar, want_grad=True)
        acc += out.cpu().numpy()
        assert torch.equal(g, gw[a:b]), (a, b)                 # a gradient row depends on its own row only: the same bits
    assert abs(acc[0] - whole[0]) <= 1e-12 * abs(whole[0])
    mass = co.dm_prior_mass_w(c, f, 0.37, train_ar=train_ar, nthreads=NTH)[0]
    assert abs(acc[1] - whole[1]) <= 1e-12 * mass[0] + 1e-14


@pytest.mark.parametrize("train_ar", [False, True])
def test_two_launches_same_bits(train_ar, mid_table):
    """bit-identical for a given grid, in the regular build too (fixed-order partials, no atomics on the sums)."""
    c, f = mid_table
    cd, fd, hd = _dc(c), _df(f), _hdev(-1.3)
    a, ga = kernels.dm_prior_wide(cd, fd, hd, train_ar=train_ar, want_grad=True)
    b, gb = kernels.dm_prior_wide(cd, fd, hd, train_ar=train_ar, want_grad=True)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert torch.equal(ga.view(torch.int64), gb.view(torch.int64))


def test_graph_replay_follows_h_in_place(mid_table):
    """h_signed is read from device memory, so one captured step follows in-place updates of h."""
    c, f = mid_table
    c, f = c[:150_001], f[:150_001]
    cd, fd = _dc(c), _df(f)
    h_dev = _hdev(0.0)
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    kernels.dm_prior_wide(cd, fd, h_dev, want_grad=True, out=out)     # workspace and library set up before capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, g_cap = kernels.dm_prior_wide(cd, fd, h_dev, want_grad=True, out=out)
    for h_s in (-1.0, 0.5, 3.0):
        h_dev.fill_(h_s)
        graph.replay()
        torch.cuda.synchronize()
        got, g = out.cpu().numpy().copy(), g_cap.clone()
        eager, ge = kernels.dm_prior_wide(cd, fd, _hdev(h_s), want_grad=True)
        assert got.tobytes() == eager.cpu().numpy().tobytes(), (h_s, got, eager)
        assert torch.equal(g.view(torch.int64), ge.view(torch.int64)), h_s
        bad = _errors(got, g.cpu().numpy(), c, f, h_s, False, True, h_s)
        assert not bad, bad


# ------------------------------------------------------------------ evaluation, W = 21
H13 = [0.02, 0.05, 0.1, 0.2, 0.37, 0.6, 1.0, 1.7, 3.0, 5.0, 9.0, 20.0, 50.0]
VAN5 = [0.01, 0.1, 1.0, 10.0, 100.0]


def _eval_check(test, train, prior, hs, van, row_base, seed=3, with_ar=True):
    n = len(test)
    got = kernels.evaluate_wide(_dc(test), _df(prior) if prior is not None else None, hs, van,
                                _dc(train) if train is not None else None, with_ar=with_ar, noise_seed=seed,
                                row_base=row_base).cpu().numpy()
    fw = prior if prior is not None else np.ones(test.shape)
    w = o.evaluation_step(test, fw, np.array(hs if hs else [1.0]), van, train, rng=HashNoiseW(seed, row_base, n, test.shape[1]))
    H, V = len(hs), len(van)
    ll_h, ll_arm, ll_v = got[:H], got[H], got[H + 1:H + 1 + V]
    cor_h, cor_arm, cor_v = got[H + V + 1:2 * H + V + 1], got[2 * H + V + 1], got[2 * H + V + 2:2 * H + 2 * V + 2]
    if H:
        assert np.allclose(ll_h, w[0], rtol=ELBO_RTOL, atol=0), (ll_h, w[0])
        np.testing.assert_array_equal(cor_h, w[3])
    assert np.allclose(ll_v, w[2], rtol=ELBO_RTOL, atol=0), (ll_v, w[2])
    np.testing.assert_array_equal(cor_v, w[5])
    if with_ar:
        assert np.isclose(ll_arm, w[1], rtol=ELBO_RTOL, atol=0) and cor_arm == w[4], (ll_arm, w[1], cor_arm, w[4])
    else:
        assert ll_arm == 0.0 and cor_arm == 0.0
    assert got[-1] == w[6]
    return got


@pytest.fixture(scope="module")
def prot_eval():
    _, counts = make_prot_table(seed=9, n=1500, num_ds=2)
    return counts[1], counts[0], prior_rows_wide(1500, 21, "softmax", seed=9)


def test_eval_wide_18_models(prot_eval):
    test, train, f = prot_eval
    assert len(H13) + len(VAN5) > 2 * 8                        # EVS_CHUNK = 8 models per launch: three launches
    for tr in (train, None):
        _eval_check(test, tr, f, H13, VAN5, row_base=77)


def test_eval_wide_without_prior_or_train(prot_eval):
    test, train, _ = prot_eval
    _eval_check(test, train, None, [], VAN5, row_base=5, with_ar=False)
    _eval_check(test, None, None, [], VAN5, row_base=5, with_ar=False)


def test_eval_wide_large_row_base(prot_eval):
    test, train, f = prot_eval
    _eval_check(test, train, f, H13[:5], VAN5[:4], row_base=2 ** 40 + 3)     # cell keys row * 21 + letter above 2^45


def test_eval_wide_ties():
    """No training counts and uniform priors: every model draws among all 21 letters, so every accuracy is the noise's."""
    _, counts = make_prot_table(seed=13, n=2000, num_ds=1)
    test = counts[0]
    f = np.full(test.shape, 1.0 / 21)
    _eval_check(test, np.zeros_like(test), f, H13, VAN5, row_base=1000, seed=8)


def test_eval_wide_grid_stride():
    n = 300_003
    tiles, grid = -(-n // EVW_ROWS), _cu() * EVAL_BLOCKS_PER_CU
    assert tiles > grid, (tiles, grid)                          # some blocks take a second tile
    c = wide_scale_table(n, 21, seed=77)
    test = c // 3
    f = prior_rows_wide(n, 21, "softmax", seed=77)
    _eval_check(test, c, f, [0.05, 0.4, 3.0, 12.0, 40.0], [0.1, 1.0, 10.0, 30.0], row_base=123)


def _parity_eval_case(case):
    """The inputs of test_parity_gpu.test_eval_kernel_parity."""
    if case == "sparse":
        tr, te, _ = sparse_table(20011, 3)
    elif case == "ties":
        te, _, _ = sparse_table(5000, 9)
        tr = np.zeros_like(te)
    else:
        tr, _ = CASES_REF["edge"]()
        te = tr[::-1].copy()
    f = prior_rows(len(te), 4, 1.0) if case != "ties" else np.full((len(te), 5), 0.2)
    return te, tr, f


@pytest.mark.parametrize("case", ["ties", "edge", "sparse"])
def test_eval_w5_twin_matches_bear_eval(case):
    te, tr, f = _parity_eval_case(case)
    d_te, d_tr, d_f = _dc(te), _dc(tr), _df(f)
    for hs, van in (([0.05, 1.0, 37.0], [0.1, 1.0, 10.0]), (H13, VAN5)):
        for t in (d_tr, None):
            want = kernels.evaluate(d_te, d_f, hs, van, t, noise_seed=77, row_base=1000).cpu().numpy()
            got = kernels.evaluate_wide(d_te, d_f, hs, van, t, noise_seed=77, row_base=1000).cpu().numpy()
            k = len(hs) + len(van) + 1
            assert np.allclose(got[:k], want[:k], rtol=1e-12, atol=0), (case, got[:k], want[:k])
            np.testing.assert_array_equal(got[k:], want[k:])
