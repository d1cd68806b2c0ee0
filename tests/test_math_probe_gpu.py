"""The device math routines one at a time (bear_math_probe_f64: the routine the production kernels call, on tables staged as they
stage them), value by value against mpmath at 40 digits or more.  A whole-kernel parity sums 1e3 .. 1e7 items and accepts 1e-11 of
the total: one bad table entry, a wrong tie of the argument reduction or a typo in a high Stirling coefficient passes it.

Every bound below comes from the routine's own arithmetic or from the claim in bear_math.h, never from what the device gave; the
observed maxima (MI355X) stand beside them and in DESIGN.md ("The math routines, one at a time")."""
import functools
import math

import mpmath as mp
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
U = 2.0 ** -53


def _probe(op, a, b=None):
    from bear_amd import kernels
    da = torch.from_numpy(np.array(a, dtype=np.float64)).to(DEV)                   # (a copy: the shared reference grids are read-only)
    if b is None:
        return kernels.math_probe(op, da).cpu().numpy()
    D, P = kernels.math_probe(op, da, torch.from_numpy(np.array(b, dtype=np.float64)).to(DEV))
    return D.cpu().numpy(), P.cpu().numpy()


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)))


def _abs_err(got, want):
    """|got - want| element by element, the difference taken at the working precision of mpmath (want: mpf values)."""
    return np.array([float(abs(mp.mpf(float(g)) - w)) if np.isfinite(g) else np.inf for g, w in zip(got, want)])


def _hold(name, err, unit, bound, x):
    """max(err / unit) <= bound, printing the observed maximum (pytest -s) and naming the worst input when it fails."""
    ratio = err / unit
    k = int(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)))
    print("observed %s: %.3g (bound %g) at %r" % (name, ratio[k], bound, float(x[k])))
    assert np.all(ratio <= bound), (name, float(x[k]), float(ratio[k]), bound, int((~(ratio <= bound)).sum()))


def _neighbours(v, k=1):
    v = np.asarray(v, dtype=np.float64)
    out = [v]
    lo, hi = v, v
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


# ---------------------------------------------------------------------------------------------------------------- bear_rcp
RCP_ULP = 1.0       # bear_math.h's claim: the last FMA rounds once, the residual after two Newton steps is ~2^-92.  Observed: 0.50


def test_rcp():
    rng = np.random.default_rng(1)
    ms = np.r_[1.0, np.nextafter(1.0, 2.0), 1.5, np.nextafter(2.0, 1.0), 1.0 + rng.random(8)]
    es = np.arange(-1020, 1021, 15)
    x = np.ldexp(ms[:, None], es[None, :]).ravel()
    x = np.r_[x, np.ldexp(1.0 + rng.random(12000), rng.integers(-1020, 1021, 12000))]
    x = np.r_[x, -x]
    mp.mp.dps = 40
    want = [1 / mp.mpf(float(v)) for v in x]
    got = _probe("rcp", x)
    _hold("bear_rcp [ulp of 1/x]", _abs_err(got, want), _ulp([float(w) for w in want]), RCP_ULP, x)


# ---------------------------------------------------------------------------------------------------------------- bear_log_tab
# four units of 2^-53 max(|log p|, 1), where table rounding, one add, the final FMA and the 3e-18 polynomial give under two; covers the
# known ~1e-16 at p = 1.  Observed: 1.7 units (1.88e-16 at p = 2.78125)
LOG_TAB_BOUND = 2.0 ** -51


def _log_tab_points():
    i = np.arange(128, dtype=np.float64)
    first, nxt, mid = (128 + i) / 256, (129 + i) / 256, (128.5 + i) / 256
    m = np.r_[first, np.nextafter(nxt, 0.0), _neighbours(mid)]                     # mantissas in [0.5, 1)
    # p = m 2^(E + 1) lies in [2^E, 2^(E + 1)): subnormal binades (ldexp rounds the mantissa to the bits that are left), the edges
    E = [-1074, -1073, -1071, -1068, -1067, -1060, -1049, -1036, -1023, -1022, -1, 0, 1, 1023]
    p = np.concatenate([np.ldexp(m, e + 1) for e in E])
    one = [1.0]
    for _ in range(4):
        one = [np.nextafter(one[0], 0.0)] + one + [np.nextafter(one[-1], 2.0)]
    p = np.r_[p, one, np.finfo(np.float64).max, 5e-324]
    rng = np.random.default_rng(2)
    p = np.r_[p, np.ldexp(0.5 + 0.5 * rng.random(8000), rng.integers(-1073, 1025, 8000))]
    p = np.unique(p[(p > 0) & np.isfinite(p)])
    assert (p < 2.0 ** -1022).sum() > 1000 and p[0] == 5e-324
    return p


def test_log_tab():
    p = _log_tab_points()
    mp.mp.dps = 40
    want = [mp.log(mp.mpf(float(v))) for v in p]
    got = _probe("log_tab", p)
    unit = np.maximum(np.abs(np.array([float(w) for w in want])), 1.0)
    _hold("bear_log_tab [max(|log p|, 1)]", _abs_err(got, want), unit, LOG_TAB_BOUND, p)
    assert np.array_equal(got.view(np.uint64), _probe("log_tab_v", p).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- bear_log1p_small
LOG1P_SMALL_ABS = 3e-18      # bear_math.h's claim for the polynomial, + 1 ulp of the result for the last FMA.  Observed: 0.63 of the bound


def test_log1p_small():
    rng = np.random.default_rng(3)
    pw = 2.0 ** -np.arange(8, 61, dtype=np.float64)
    t = np.r_[_neighbours(pw, 2), 0.0, 5e-324, 1e-300, 2.0 ** -8 * rng.random(12000), 2.0 ** -(8 + 52 * rng.random(8000))]
    t = t[t <= 2.0 ** -8]
    t = np.r_[t, -t]
    assert 2.0 ** -8 in t and -2.0 ** -8 in t and 2.0 ** -60 in t and -2.0 ** -60 in t and 0.0 in t
    mp.mp.dps = 40
    want = [mp.log1p(mp.mpf(float(v))) for v in t]
    got = _probe("log1p_small", t)
    unit = LOG1P_SMALL_ABS + _ulp([float(w) for w in want])
    _hold("bear_log1p_small [3e-18 + 1 ulp]", _abs_err(got, want), unit, 1.0, t)
    assert np.array_equal(got.view(np.uint64), _probe("log1p_small_v", t).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- bear_log1p_pos
LOG1P_POS_ULP = 3.0          # the 1-ulp library log, the correction term, one add.  Observed: 1.02


def test_log1p_pos():
    rng = np.random.default_rng(4)
    t = np.r_[0.0, 5e-324, 1e-300, 1e300, _neighbours(2.0 ** np.arange(-60, 61, dtype=np.float64)), 2.0 ** (-60 + 120 * rng.random(15000)),
              10.0 ** (-300 + 600 * rng.random(2000))]
    mp.mp.dps = 40
    want = [mp.log1p(mp.mpf(float(v))) for v in t]
    got = _probe("log1p_pos", t)
    _hold("bear_log1p_pos [ulp]", _abs_err(got, want), _ulp([float(w) for w in want]), LOG1P_POS_ULP, t)


# ---------------------------------------------------------------------------------------------------------------- the exponentials
EXP_ULP = 2.0   # table entry (library exp2, <= 1 ulp), a degree-5 polynomial on |r| <= ln2 / 256 (truncation 2e-18 relative), one FMA.
#                 Observed: bear_exp_tab 1.23, cnn_exp_neg 1.23, lin_exp_units 1.24
OCTAVES = (0, -1, -2, -3, -7, -64, -511, -512, -1008, -1009)      # k >> 7 of the reduction; -1009 is the last whole one above -700


@functools.lru_cache(maxsize=None)
def _exp_reference():
    """The points of the two exp(z) routines and exp at 40 digits, computed once for both."""
    z = _exp_points()
    mp.mp.dps = 40
    return z, [mp.exp(mp.mpf(float(v))) for v in z]


def _exp_points():
    mp.mp.dps = 60
    unit = mp.log(2) / 128
    K = np.concatenate([128 * q + np.arange(128) for q in OCTAVES])
    z = [float(mp.mpf(int(k)) * unit) for k in K]                                    # table points: r = 0 up to the rounding of z
    z += [float((mp.mpf(int(k)) + h) * unit) for k in K for h in (mp.mpf(-0.5), mp.mpf(0.5))]   # the ties of rint
    rng = np.random.default_rng(5)
    z = np.r_[_neighbours(z, 2), _neighbours([-700.0], 2), 0.0, -0.0, -700.0 * rng.random(5000), -rng.random(1000)]
    return np.unique(z[(z <= 0.0) & (z >= -700.0)])


def _exp_check(op, name):
    z, want = _exp_reference()
    mp.mp.dps = 40
    got = _probe(op, z)
    _hold(name + " [ulp]", _abs_err(got, want), _ulp([float(w) for w in want]), EXP_ULP, z)
    assert _probe(op, np.array([0.0, -0.0])).tolist() == [1.0, 1.0]
    return _probe(op, np.array([np.nextafter(-700.0, -np.inf), -745.0, -1e300, -np.inf, -700.0, np.nan]))


def test_exp_tab():
    tail = _exp_check("exp_tab", "bear_exp_tab")
    assert np.array_equal(tail[:4].view(np.uint64), np.zeros(4, np.uint64))          # exactly +0.0 below -700
    assert np.isnan(tail[5])


def test_cnn_exp_neg():
    tail = _exp_check("cnn_exp_neg", "cnn_exp_neg")
    assert np.array_equal(tail[:4].view(np.uint64), np.full(4, tail[4:5].view(np.uint64)[0]))     # its own value at -700
    # NaN: `z > -700 ? z : -700` turns it into exp(-700).  Recorded, not asserted (no caller can hand it one)
    print("observed cnn_exp_neg(NaN) = %r" % float(tail[5]))


def test_lin_exp_units():
    lo, hi = -700.0 * 128 / math.log(2.0), 600.0 * 128 / math.log(2.0)               # what its callers guarantee
    rng = np.random.default_rng(6)
    ints = np.concatenate([128.0 * q + np.arange(128) for q in OCTAVES + (1, 2, 511, 864)])
    d = np.r_[ints, _neighbours(np.r_[ints + 0.5, ints - 0.5], 2), 0.0, -0.0, np.floor(lo) + 1, np.floor(hi), lo, hi,
              lo + (hi - lo) * rng.random(5000), np.round(lo + (hi - lo) * rng.random(2000)), 256 * (rng.random(2000) - 0.5)]
    d = np.unique(d[(d >= lo) & (d <= hi)])
    mp.mp.dps = 40
    want = [mp.power(2, mp.mpf(float(v)) / 128) for v in d]
    got = _probe("lin_exp_units", d)
    _hold("lin_exp_units [ulp]", _abs_err(got, want), _ulp([float(w) for w in want]), EXP_ULP, d)
    assert _probe("lin_exp_units", np.array([0.0, -0.0])).tolist() == [1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------- the Stirling tails
# absolute error <= the first omitted term of the series at y, + STIR_*_ROUND units of 2^-53 of the tail.  The routines take r = 1 / y; the
# reference is the exact tail at y = 1 / r, r the double handed in.  The roundings, each <= 2^-53 of the tail: the stored coefficient
# 1/12, the last Horner FMA and the closing product -- three for lg; psi squares r first, a fourth.  Every earlier Horner step reaches
# the result through a factor r^2 <= 1/64 and a coefficient ratio <= 1/10: 1/16 of a unit covers them all.  (2^-52 of the tail, two
# units, was the first figure; three and four roundings do not fit in two.  The routines' own arithmetic, modelled with exactly
# rounded FMAs on these points, reaches 2.06 units (lg) and 2.70 (psi) -- the same operations, so the device gives the same.)
# Observed: lg 0.92, psi 0.93 of the bound (at y ~ 8.5 .. 10, where the omitted term is nearly all of it)
STIR_LG_ROUND, STIR_PSI_ROUND = 3.0 + 1.0 / 16, 4.0 + 1.0 / 16


def _stir_points():
    rng = np.random.default_rng(7)
    y = np.r_[8.0, 8.5, 9.0, 10.0, 12.0, 16.0, 32.0, 100.0, 1e3, 1e4, 1e5, 1e6, 8.0 * (1e6 / 8.0) ** rng.random(4000), 8.0 + 8.0 * rng.random(1000)]
    r = 1.0 / y
    return r[r <= 0.125]


def _stir_check(op, name, tail, omitted, units):
    r = np.r_[_stir_points(), 1e-300]
    got = _probe(op, r)
    assert np.all(np.isfinite(got))
    ratio = np.empty(len(r))
    for i, v in enumerate(r):
        mp.mp.dps = 45 + int(2.2 * -math.log10(v))             # the tail is ~1 / (12 y) (lg), 1 / (12 y^2) (psi) of terms of size y log y
        y = 1 / mp.mpf(float(v))
        w = tail(y)
        # + half the smallest subnormal: the tail of psi at y = 1e300 is 8e-602, which no double holds
        ratio[i] = float(abs(mp.mpf(float(got[i])) - w) / (omitted(y) + units * mp.mpf(2) ** -53 * abs(w) + mp.mpf(2) ** -1075))
    mp.mp.dps = 40
    _hold(name + " [first omitted term + %g * 2^-53 tail]" % units, ratio, np.ones(len(r)), 1.0, r)


def test_stir_lg():
    _stir_check("stir_lg", "bear_stir_lg", lambda y: mp.loggamma(y) - ((y - mp.mpf(0.5)) * mp.log(y) - y + mp.log(2 * mp.pi) / 2),
                lambda y: mp.mpf(3617) / 122400 * y ** -15, STIR_LG_ROUND)


def test_stir_psi():
    _stir_check("stir_psi", "bear_stir_psi", lambda y: mp.log(y) - 1 / (2 * y) - mp.digamma(y), lambda y: mp.mpf(3617) / 8160 * y ** -16,
                STIR_PSI_ROUND)


# ---------------------------------------------------------------------------------------------------------------- the wave reductions
def test_wave_reductions():
    onehot = np.eye(64).ravel()
    for op in ("wave_sum", "wave_max"):
        assert np.array_equal(_probe(op, onehot), np.ones(64 * 64)), op             # every lane sees every lane
    pw = np.r_[2.0 ** np.arange(52), np.zeros(12)]
    assert np.array_equal(_probe("wave_sum", pw), np.full(64, 2.0 ** 52 - 1))       # every partial sum is exact
    assert np.array_equal(_probe("wave_max", pw), np.full(64, 2.0 ** 51))
    rng = np.random.default_rng(8)
    v = (rng.standard_normal((200, 64)) * 10.0 ** rng.integers(-20, 20, (200, 64)))
    got = _probe("wave_sum", v.ravel()).reshape(200, 64)
    assert np.array_equal(got.view(np.uint64), np.repeat(got[:, :1], 64, 1).view(np.uint64))    # the 64 lanes agree to the bit
    want = np.array([math.fsum(row) for row in v])
    err = np.abs(got[:, 0] - want) / (64 * U * np.abs(v).sum(1))
    print("observed bear_wave_sum: %.3g of 64 * 2^-53 * sum|v|" % err.max())         # observed: 0.031
    assert np.all(err <= 1.0)
    a = np.abs(v)
    a[0, 5], a[1, :] = 0.0, 0.0
    a[1, 63], a[2, 0] = 5e-324, 1e300
    got = _probe("wave_max", a.ravel()).reshape(200, 64)
    assert np.array_equal(got, np.repeat(a.max(1)[:, None], 64, 1))                  # exact on non-negative values
    # a ragged last wave: the elements past n count as 0
    assert np.array_equal(_probe("wave_sum", np.ones(100)), np.r_[np.full(64, 64.0), np.full(36, 36.0)])
    assert np.array_equal(_probe("wave_max", np.arange(100.0)), np.r_[np.full(64, 63.0), np.full(36, 99.0)])


# ---------------------------------------------------------------------------------------------------------------- the item routines
# D = lgamma(x + c) - lgamma(x) = sum_j log(x + j), P = digamma(x + c) - digamma(x): the project's own figures, on the L1 mass of the
# sum itself (sum_j |log(x + j)| = D - 2 min(log x, 0): only the first term can be negative).  A Python model of the routine's
# arithmetic (library log, no FMA) stays within 2.9e-16 mass and 1.3e-15 relative on this grid.
# Observed, as fractions of the two bounds: the library-log forms D 8.6e-4 (3.4e-16 of the mass), P 0.013 (1.3e-15); the table-log forms
# D 0.11 (x = 1, c = 1: the table log of exactly 1.0 is 1.1e-16 against the 1e-15 floor; 1.2e-15 of the mass elsewhere) and P 0.28
# (x = 1e12, c = 2^32 - 1: r = c / x just above 2^-8, the table log's ~1e-16 against log1p(r) = 4.3e-3); at x >= 2^1000 5.5e-4 and
# 2.2e-3, and no NaN from dm_row_item
ITEM_D_MASS, ITEM_D_ABS, ITEM_P_REL = 4e-13, 1e-15, 1e-13

X_PRESENT = [1e-7, 3e-5, 0.013, 0.1 + 1e-7, 0.5, 0.999, 1.0, 1.7, 4.0, 7.99, 8.0, 8.01, 31.4, 250.0, 1e4, 1e7, 2.0 ** 30, 2.0 ** 31, 1e12]
X_GRID = ([1e-300, 1e-100, 1e-30, 1e-12] + X_PRESENT + [7.0, 7.99, 8.0, 8.01]
          + [float(np.nextafter(2.0 ** 30, 0)), 2.0 ** 30, float(np.nextafter(2.0 ** 30, np.inf)), 2.0 ** 31, 1e15]
          + [float(np.nextafter(2.0 ** 60, 0)), 2.0 ** 60, float(np.nextafter(2.0 ** 60, np.inf)), 2.0 ** 61, 1e30, 1e100, 2.0 ** 999])
C_GRID = [1, 2, 15, 16, 17, 18, 24, 25, 31, 32, 64, 65, 100, 1000, 254715, 10 ** 7, 2 ** 32 - 1, 2 ** 32, 5 * (2 ** 32 - 1), 2 ** 40]
X_HUGE = [2.0 ** 1000, 2.0 ** 1010, 2.0 ** 1021, 2.0 ** 1022, 2.0 ** 1023, float(np.finfo(np.float64).max)]      # [2^1000, inf)
SRT_ROUTINES = ("srt_general", "srt_general_fast", "srt_general_auto")
ROW_ROUTINES = ("row_item_tab", "row_item")


def _item_reference(X, C):
    Dw, Pw = np.empty(len(X)), np.empty(len(X))
    for i, (x, c) in enumerate(zip(X, C)):
        # digits to spare behind the cancellation of the two values, ~x / c of them (at 50 digits the digamma difference at 2^999 is 0)
        mp.mp.dps = 50 if x <= 1.0 else int(50 + 2.2 * math.log10(x))
        a, b = mp.mpf(float(x)), mp.mpf(float(x)) + int(c)
        Dw[i], Pw[i] = float(mp.loggamma(b) - mp.loggamma(a)), float(mp.digamma(b) - mp.digamma(a))
    mp.mp.dps = 40
    return Dw, Pw


def _item_grid(xs):
    X, C = np.meshgrid(np.array(sorted(set(xs))), np.array(C_GRID, dtype=np.float64), indexing="ij")
    return X.ravel(), C.ravel()


@pytest.fixture(scope="module")
def items():
    X, C = _item_grid(X_GRID)
    Dw, Pw = _item_reference(X, C)
    for a in (X, C, Dw, Pw):
        a.setflags(write=False)
    assert np.all(np.isfinite(Dw)) and np.all(Pw > 0)
    return X, C, Dw, Pw


def _item_errors(D, P, X, Dw, Pw):
    mass = Dw - 2.0 * np.minimum(np.log(X), 0.0)
    return np.abs(D - Dw) / (ITEM_D_MASS * mass + ITEM_D_ABS), np.abs(P - Pw) / (ITEM_P_REL * np.abs(Pw))


def _item_hold(name, D, P, X, C, Dw, Pw, nan_ok=False):
    """Within the bounds -- or, with nan_ok, NaN in both results: never a finite wrong number."""
    eD, eP = _item_errors(D, P, X, Dw, Pw)
    nan = np.isnan(D) & np.isnan(P) if nan_ok else np.zeros(len(X), bool)
    ok = nan | ((eD <= 1.0) & (eP <= 1.0))
    if (~nan).any():
        print("observed %s: D %.3g, P %.3g of their bounds%s" % (name, eD[~nan].max(), eP[~nan].max(),
                                                                  ", %d of %d NaN" % (nan.sum(), len(X)) if nan_ok else ""))
    k = int(np.argmax(~ok))
    assert ok.all(), (name, float(X[k]), float(C[k]), float(D[k]), float(Dw[k]), float(P[k]), float(Pw[k]), int((~ok).sum()))


@pytest.mark.parametrize("op", SRT_ROUTINES + ROW_ROUTINES)
def test_item_routines_whole_domain(op, items):
    X, C, Dw, Pw = items
    D, P = _probe(op, X, C)
    _item_hold(op, D, P, X, C, Dw, Pw)


@pytest.mark.parametrize("path", [0, 1, 2])
def test_item_entry_whole_domain(path, items):
    """The same grid through bear_dm_items_f64 (path 0: the product path of srt_light for c <= 24; 1 / 2: srt_general[_fast]), for the
    counts that fit its uint32."""
    from bear_amd import kernels
    X, C, Dw, Pw = items
    k = C < 2.0 ** 32
    dx = torch.from_numpy(X[k]).to(DEV)
    dc = torch.from_numpy(C[k].astype(np.uint32).view(np.int32)).to(DEV)
    D, P = kernels.dm_items(dx, dc, path=path)
    _item_hold("bear_dm_items_f64 path %d" % path, D.cpu().numpy(), P.cpu().numpy(), X[k], C[k], Dw[k], Pw[k])


def test_item_routines_from_2_1000():
    """x in [2^1000, inf): srt_general_fast answers NaN by design; the routines that choose it for a finite x (srt_general_auto, the
    rows family's dm_row_item with the table) give the right value or NaN; the library forms give the right value."""
    X, C = _item_grid(X_HUGE)
    Dw, Pw = _item_reference(X, C)
    D, P = _probe("srt_general_fast", X, C)
    assert np.isnan(D).all() and np.isnan(P).all()
    for op in ("srt_general_auto", "row_item_tab"):
        D, P = _probe(op, X, C)
        _item_hold(op + " at x >= 2^1000", D, P, X, C, Dw, Pw, nan_ok=True)
    for op in ("srt_general", "row_item"):
        D, P = _probe(op, X, C)
        _item_hold(op + " at x >= 2^1000", D, P, X, C, Dw, Pw)


def test_item_routines_out_of_domain():
    """x = 0, x < 0 and NaN give NaN from every routine that documents it (sorted_common.h: the srt_general family)."""
    bad = np.repeat([0.0, -0.0, -1.0, np.nan, -np.inf], 3)
    c = np.tile([1.0, 17.0, 2.0 ** 33], 5)
    for op in SRT_ROUTINES:
        D, P = _probe(op, bad, c)
        assert np.isnan(D).all() and np.isnan(P).all(), op
