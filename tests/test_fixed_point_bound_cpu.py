"""The inequality the fixed-point gradient tables of BEAR_AMD_DETERMINISTIC rest on (kernels_linear.h, lin_fx_scale): a cell's
w = f u P(f u + eps, c), P(x, c) = digamma(x + c) - digamma(x), never exceeds min(c, 1 + u (1 + ln c)) -- so the sum of |g| over
everything added into one gradient stays below `bound` and bound 2^-62 is a safe unit for a 64-bit table.  Checked with mpmath at 50
digits (the ratio comes within 1e-16 of one: double precision cannot assert it); no GPU."""
import itertools

import mpmath as mp
import pytest

EPSILON = 1e-7          # bear_amd.kernels.EPSILON (asserted below without loading the library's bindings twice)

US = [1e-8, 1e-5, 1e-3, 0.1, 1.0, 12.0, 1e3, 1e6]
CS = [1, 2, 3, 24, 25, 1000, 254715, 10 ** 7, 2 ** 30, 4 * 10 ** 9]
FS = [1e-300, 1e-100, 1e-30, 1e-12, 1e-6, 1e-3, 0.2, 0.5, 1.0 - 1e-9, 1.0]
EPSS = [1e-300, 1e-100, 1e-30, 1e-15, 1e-10, EPSILON]


def test_epsilon_is_the_librarys():
    from bear_amd import kernels
    assert kernels.EPSILON == EPSILON


@pytest.mark.parametrize("u", US)
def test_cell_gradient_never_exceeds_the_bound(u):
    worst = mp.mpf(0)
    with mp.workdps(50):
        for c, f, eps in itertools.product(CS, FS, EPSS):
            x = mp.mpf(f) * mp.mpf(u) + mp.mpf(eps)
            w = mp.mpf(f) * mp.mpf(u) * (mp.digamma(x + c) - mp.digamma(x))
            bound = min(mp.mpf(c), 1 + mp.mpf(u) * (1 + mp.log(c)))
            ratio = w / bound
            worst = max(worst, ratio)
            assert w >= 0 and ratio <= 1 + mp.mpf(10) ** -12, (u, c, f, eps, mp.nstr(ratio, 20))
    assert worst > mp.mpf("0.05"), (u, mp.nstr(worst, 10))          # (the grid does come near the bound: the check is not vacuous)
