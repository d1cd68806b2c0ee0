"""The four row kernels (kernels_rows.h) with more tiles than blocks.  Their grid is capped at 2 blocks of 1024-row tiles or 4 blocks
of 512-row tiles per CU -- 524 288 rows on 256 CUs either way -- and no other test gives them more: the `tile += gridDim.x` pass of the
tile loop, and the barrier that opens a block's second tile over LDS its threads may still be reading, ran untested.  N rows here
are 1075 / 2149 tiles: every block takes two to three of them, the last tile is partial, and N is odd, so the staged dword
stream ends in a tail shorter than 16 bytes.  Against the oracle at the tolerances of test_parity_gpu.py (test_dm_prior_parity,
test_reference_aware_plan_parity); and the gradient rows of a slice run alone equal the full run's bit for bit (rows are
independent: only the tile and the pass in which a row is met differ)."""
import os

import numpy as np
import pytest
import torch

import c_oracle as co
from util import dense_table, prior_rows

pytestmark = pytest.mark.gpu

N = 1_100_003
SLICE0, SLICE_ROWS = 786_940, 4_099        # met in the blocks' second pass; starts at a multiple of 4 rows (16-byte aligned slabs)
H_S = -0.3
REF_ARGS = (0.0, float(np.log(1 / 30)), float(-np.log(100)))
ELBO_RTOL = 1e-11                          # test_parity_gpu.py
MASS_RTOL = float(os.environ.get("BEAR_TEST_MASS_RTOL", "2e-13"))


def _close(got, want, rtol):
    assert abs(got - want) <= rtol * max(abs(want), 1e-300), (got, want, abs(got - want) / max(abs(want), 1e-300))


def _mass_close(got, want, mass, what):
    assert abs(got - want) <= MASS_RTOL * mass + 1e-14, (what, got, want, abs(got - want) / max(mass, 1e-300))


@pytest.fixture(scope="module")
def table():
    """A dense table of N rows on the host and the device, and the oracle's answers for it (computed once, never modified)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda", 0)
    tr, rf = dense_table(N, 31)
    f = prior_rows(N, 5)
    t = {"tr": tr, "rf": rf, "f": f, "dev": dev}
    for k in ("tr", "rf"):
        t["d_" + k] = torch.from_numpy(t[k].view(np.int32)).to(dev)
    t["d_f"] = torch.from_numpy(f).to(dev)
    for ar in (False, True):
        t["prior", ar] = co.dm_prior(tr, f, H_S, train_ar=ar, want_grad=True, nthreads=4)
        t["ref", ar] = co.dm_ref(tr, rf, *REF_ARGS, train_ar=ar, nthreads=4)
        t["ref_mass", ar] = co.dm_ref_mass(tr, rf, *REF_ARGS, train_ar=ar, nthreads=4)
    t["prior_mass"] = co.dm_prior_mass(tr, f, H_S, nthreads=4)
    return t


def _check_prior(t, train_ar, out, grad, what):
    want, wantg = t["prior", train_ar]
    out, g = out.cpu().numpy(), grad.cpu().numpy()
    _close(out[0], want[0], ELBO_RTOL)
    if train_ar:
        assert out[1] == 0.0 and want[1] == 0.0       # no h in the multinomial
    else:
        _mass_close(out[1], want[1], t["prior_mass"], what)
    assert np.allclose(g, wantg, rtol=1e-9, atol=1e-9 * np.abs(wantg).max()), (what, np.abs(g - wantg).max())


def _slice(x):
    return x[SLICE0:SLICE0 + SLICE_ROWS]


@pytest.mark.parametrize("train_ar", [False, True])
def test_dm_prior_kernel_wraps(train_ar, table):
    from bear_amd import kernels
    t = table
    out, g = kernels.dm_prior(t["d_tr"], t["d_f"], H_S, train_ar=train_ar, want_grad=True)
    _check_prior(t, train_ar, out, g, ("dm_prior", train_ar))
    _, g_part = kernels.dm_prior(_slice(t["d_tr"]), _slice(t["d_f"]), H_S, train_ar=train_ar, want_grad=True)
    assert torch.equal(g_part, _slice(g))


@pytest.mark.parametrize("train_ar", [False, True])
def test_dm_prior_rows_kernel_wraps(train_ar, table):
    from bear_amd import kernels
    t = table
    plan = kernels.Plan(t["d_tr"], 5, rows_if_dense=True)
    assert plan.rowwise
    out, g = kernels.dm_prior_planned(plan, t["d_f"], H_S, want_grad=True, train_ar=train_ar)
    _check_prior(t, train_ar, out, g, ("dm_prior_planned", train_ar))
    part = kernels.Plan(_slice(t["d_tr"]), 5, rows_if_dense=True)
    assert part.rowwise
    _, g_part = kernels.dm_prior_planned(part, _slice(t["d_f"]), H_S, want_grad=True, train_ar=train_ar)
    assert torch.equal(g_part, _slice(g))


def _check_ref(t, train_ar, got, what):
    want, mass = t["ref", train_ar], t["ref_mass", train_ar]
    got = got.cpu().numpy()
    _close(got[0], want[0], ELBO_RTOL)
    for k in range(1, 4):
        _mass_close(got[k], want[k], mass[k - 1], (what, k))


@pytest.mark.parametrize("train_ar", [False, True])
def test_dm_ref_kernel_wraps(train_ar, table, monkeypatch):
    from bear_amd import kernels
    t = table
    if not train_ar:
        monkeypatch.setenv("BEAR_ROWS_KERNEL", "1")      # BEAR mode: the row kernel instead of the sorted one
    _check_ref(t, train_ar, kernels.dm_ref(t["d_tr"], t["d_rf"], *REF_ARGS, train_ar=train_ar), ("dm_ref", train_ar))


@pytest.mark.parametrize("train_ar", [False, True])
def test_dm_ref_rows_kernel_wraps(train_ar, table):
    from bear_amd import kernels
    t = table
    plan = kernels.Plan(t["d_tr"], 4, ref=t["d_rf"])
    assert plan.nbytes < 64 * 1024                       # the dense form: histograms only
    _check_ref(t, train_ar, kernels.dm_ref_planned(plan, t["d_rf"], *REF_ARGS, train_ar=train_ar), ("dm_ref_planned", train_ar))
