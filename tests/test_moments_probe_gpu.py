"""bear_psi and bear_psi1 (bear_math.h: the digamma and trigamma of one argument under kernels_moments.h) through
bear_math_probe_f64, value by value against mpmath at 50 digits, the way tests/test_math_probe_gpu.py holds the other routines.

Both bounds come from the routines' own arithmetic (DESIGN.md 3.1 has the derivation and the observed maxima), never from what the
device gave.  With u = 2^-53, m = the shift's steps (ceil(8 - x) below 8, else 0), y = x + m, S = sum_{j<m} 1 / (x + j) and
S2 = sum_{j<m} 1 / (x + j)^2:

  psi:   |err| <= u ((2 m + 1) S + 4 log y + 2 + |psi(x)|) + 3617/8160 y^-16
         the reciprocals as p'/p: m - 1 products, m - 1 FMAs of p' at full weight (every term is positive), x + j, the reciprocal
         and the product, 2 m + 1 roundings of S;  log y to 1 ulp (2 u relative) and the two subtractions that form psi(y), 4 u
         log y;  the rounding of y through psi'(y) y <= 1.07, the halved reciprocal and the tail's own roundings (4.06 u of
         1 / (12 y^2)), 2 u absolute;  the closing subtraction, u |psi(x)|;  the first omitted term of bear_stir_psi.  Near the root
         1.4616... S and psi(y) cancel: the bound is absolute there, against those two magnitudes (~2.0 each), not against psi.
  psi1:  |err| <= u ((m + 4) S2 + 4 psi1(y) + psi1(x)) + 174611/330 y^-21
         every term is positive: per reciprocal x + j and bear_rcp twice over (the square), 4 u of the term, and m FMA
         accumulations at full weight;  psi1(y): the rounding of y, the reciprocal, the FMA and the two additions, 4 u;  the closing
         addition;  the first omitted term of bear_stir_psi1 (4.3e-16 of psi1(8)).

Observed (MI355X): psi 0.68 of its bound (2.0e-15 at x = 8.0002, the omitted term), 1.7e-15 absolute within 1e-9 of the root; psi1
0.58 of its bound (7.5e-17 at x = 7.10)."""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
U = mp.mpf(2) ** -53
ROOT_PSI = 1.4616321449683623            # psi's positive root
TSTIR = 8.0                              # BEAR_TSTIR


def _probe(op, a):
    from bear_amd import kernels
    return kernels.math_probe(op, torch.from_numpy(np.array(a, dtype=np.float64)).to(DEV)).cpu().numpy()


def _neighbours(v, k):
    v = np.asarray(v, dtype=np.float64)
    out, lo, hi = [v], v, v
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def _points():
    """2^-40 .. 2^60 log-uniform, the integers 1 .. 9, a band round BEAR_TSTIR (the shift's last step comes and goes; every integer
    below it is a step too), a band round the root."""
    rng = np.random.default_rng(21)
    x = np.r_[2.0 ** (-40 + 100 * rng.random(6000)), 2.0 ** -40, 2.0 ** 60, np.arange(1.0, 10.0), _neighbours(np.arange(1.0, 10.0), 2),
              _neighbours([TSTIR], 40), TSTIR + 0.02 * (rng.random(600) - 0.5), 7.0 + 2.0 * rng.random(600),
              _neighbours([ROOT_PSI], 40), ROOT_PSI + 2e-3 * (rng.random(600) - 0.5), ROOT_PSI + 2e-9 * (rng.random(200) - 0.5)]
    return np.unique(x)


def _steps(x):
    need = TSTIR - x                      # as the routines form it, in double
    return int(math.ceil(need)) if need > 0.0 else 0


def _hold(name, got, want, bound, x):
    ratio = np.array([float(abs(mp.mpf(float(g)) - w) / b) if np.isfinite(g) else np.inf for g, w, b in zip(got, want, bound)])
    k = int(np.argmax(ratio))
    print("observed %s: %.3g of the bound at %r (error %.3g)" % (name, ratio[k], float(x[k]), float(abs(mp.mpf(float(got[k])) - want[k]))))
    assert np.all(ratio <= 1.0), (name, float(x[k]), float(ratio[k]), int((ratio > 1.0).sum()))
    return ratio


@pytest.fixture(scope="module")
def reference():
    x = _points()
    assert x.min() == 2.0 ** -40 and x.max() == 2.0 ** 60 and (np.abs(x - ROOT_PSI) < 1e-9).sum() > 100 and (x == TSTIR).any()
    rows = []
    with mp.workdps(50):
        for v in x.tolist():
            X, m = mp.mpf(v), _steps(v)
            y = X + m
            S = mp.fsum(1 / (X + j) for j in range(m))
            S2 = mp.fsum(1 / (X + j) ** 2 for j in range(m))
            w0, w1 = mp.digamma(X), mp.polygamma(1, X)
            b0 = U * ((2 * m + 1) * S + 4 * abs(mp.log(y)) + 2 + abs(w0)) + mp.mpf(3617) / 8160 * y ** -16
            b1 = U * ((m + 4) * S2 + 4 * mp.polygamma(1, y) + w1) + mp.mpf(174611) / 330 * y ** -21
            rows.append((w0, w1, b0, b1, max(S, abs(mp.digamma(y)))))
    return x, rows


def test_psi(reference):
    x, rows = reference
    with mp.workdps(50):
        got = _probe("psi", x)
        _hold("bear_psi", got, [r[0] for r in rows], [r[2] for r in rows], x)
        # what the bound amounts to: within 30 u of the larger of the two magnitudes that cancel (S and psi(y)), + the omitted term
        loose = [30 * U * r[4] + mp.mpf(3617) / 8160 * mp.mpf(TSTIR) ** -16 for r in rows]
        assert all(r[2] <= b for r, b in zip(rows, loose))
        near = np.abs(x - ROOT_PSI) < 1e-9
        err = np.array([float(abs(mp.mpf(float(g)) - r[0])) for g, r in zip(got[near], [r for r, n in zip(rows, near) if n])])
        print("observed bear_psi within 1e-9 of its root: largest |error| = %.3g (|psi| there <= %.3g)" % (err.max(), np.abs(got[near]).max()))


def test_psi1(reference):
    x, rows = reference
    with mp.workdps(50):
        got = _probe("psi1", x)
        assert (got > 0).all()
        _hold("bear_psi1", got, [r[1] for r in rows], [r[3] for r in rows], x)
        rel = max(float(r[3] / r[1]) for r in rows)
        print("the bound of bear_psi1 is at most %.3g = %.1f u of psi1" % (rel, rel * 2.0 ** 53))
        assert rel <= 20 * 2.0 ** -53                      # (m + 4) + 4 + 1 roundings and 3.9 u of omitted term at y = 8
