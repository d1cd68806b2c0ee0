"""The general mode-N planned step (prior rows not asserted normalised) takes the context terms of every context from the plan's
histogram and only checks the row sums per tile: a row whose sum fails the |S - 1| test swaps its shared term for its own, with
its total read from the tile's nrow bytes in LDS (staged behind a tile with a failing row) or from the plan in HBM.  These tests
put failing rows where each of those paths is taken and hold the result to the oracle and to the unplanned kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import c_oracle as co

pytestmark = pytest.mark.gpu

ELBO_RTOL = 1e-11
MASS_RTOL = 2e-13
TOL = 4.5e-16          # SRT_SUM1_TOL of kernels_sorted.h
H_SIGNED = -0.3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def table(dev):
    """A k-mer table with several tiles per block of the step's grid, its plan and softmax prior rows."""
    from bear_amd import kernels
    n = 3_000_000
    tr = kernels.synth_counts(11, 0, n, dev, want=("train",))["train"]
    plan = kernels.Plan(tr, 5)
    f = kernels.synth_prior(11, 0, n, dev).cpu().numpy()
    return tr, plan, f


def _kernel_sum(f):
    """The row sums in the kernel's order of summation."""
    return ((f[:, 0] + f[:, 1]) + (f[:, 2] + f[:, 3])) + f[:, 4]


def _block_tiles(plan, dev):
    """Tile ranges [first, end) of the blocks of the planned step's grid (one block per CU, as grid_plan)."""
    row0, rows, _, _ = plan.tiles()
    t = len(row0)
    g = max(1, min(torch.cuda.get_device_properties(dev).multi_processor_count, t))
    return row0.astype(np.int64), rows.astype(np.int64), [(t * b // g, t * (b + 1) // g) for b in range(g)]


def _check(tr, plan, f, dev, what, normalized_too=False):
    from bear_amd import kernels
    c = tr.cpu().numpy().view(np.uint32)
    d_f = torch.from_numpy(np.ascontiguousarray(f)).to(dev)
    want, _ = co.dm_prior(c, f, H_SIGNED, nthreads=8)
    mass = co.dm_prior_mass(c, f, H_SIGNED, nthreads=8)
    got = kernels.dm_prior_planned(plan, d_f, H_SIGNED).cpu().numpy()
    unpl, _ = kernels.dm_prior(tr, d_f, H_SIGNED)
    unpl = unpl.cpu().numpy()
    outs = [("planned", got), ("unplanned", unpl)]
    if normalized_too:
        outs.append(("normalized", kernels.dm_prior_planned(plan, d_f, H_SIGNED, normalized=True).cpu().numpy()))
    for name, o in outs:
        assert abs(o[0] - want[0]) <= ELBO_RTOL * abs(want[0]), (what, name, o[0], want[0])
        assert abs(o[1] - want[1]) <= MASS_RTOL * mass + 1e-14, (what, name, o[1], want[1], mass)
    assert abs(got[0] - unpl[0]) <= ELBO_RTOL * abs(unpl[0]), (what, got[0], unpl[0])
    return got


def test_softmax_rows(table, dev):
    tr, plan, f = table
    live = tr.cpu().numpy().astype(np.int64).sum(1) > 0
    assert np.all(np.abs(_kernel_sum(f[live]) - 1.0) <= TOL)   # every context with counts takes the shared term
    _check(tr, plan, f, dev, "softmax", normalized_too=True)


def test_rows_not_normalised(table, dev):
    """bench.py's net_rows_not_normalised rows: every row fails the test (nrow staged from a block's third tile on)."""
    tr, plan, f = table
    n = f.shape[0]
    scale = 1.0 + 1e-3 * ((np.arange(n, dtype=np.int64) * 2654435761 % 1000003).astype(np.float64) / 1000003.0)
    _check(tr, plan, f * scale[:, None], dev, "scaled")


def test_failing_rows_sprinkled(table, dev):
    """Softmax rows with a few unnormalised ones: in the first tile of a block, in middle tiles after clean tiles (the tile's nrow
    bytes read from HBM) and two tiles behind a failing one (staged in LDS), and in the table's last tile."""
    tr, plan, f = table
    row0, rows, blocks = _block_tiles(plan, dev)
    long_blocks = [b for b, (s, e) in enumerate(blocks) if e - s >= 6]
    assert len(long_blocks) >= 2, "the table is too small for the grid"
    picks = [blocks[long_blocks[0]][0],                    # first tile of a block
             blocks[long_blocks[1]][0] + 3,                # after three clean tiles: nrow not staged
             blocks[long_blocks[1]][0] + 5,                # two tiles behind a failing one: nrow staged
             len(row0) - 1]                                # the table's last tile
    rng = np.random.default_rng(5)
    counts = tr.cpu().numpy()
    tot = counts.astype(np.int64).sum(1)
    g = f.copy()
    for t in picks:
        r = np.arange(row0[t], row0[t] + rows[t])
        live = r[(tot[r] > 0) & (tot[r] <= 24)]
        sel = np.concatenate([rng.choice(live, size=min(40, len(live)), replace=False), r[:1], r[-1:]])
        g[sel] *= 1.0 + 1e-3 * (0.5 + rng.random((len(sel), 1)))
        assert np.all(np.abs(_kernel_sum(g[sel]) - 1.0) > TOL)
    _check(tr, plan, g, dev, "sprinkled")


def _nudge(f, target):
    """f with its last column moved so that the kernel's row sum is exactly `target` (and the rows where that worked)."""
    g = f.copy()
    for _ in range(16):
        s = _kernel_sum(g)
        off = s != target
        if not off.any():
            break
        g[off, 4] += target - s[off]
    return g, _kernel_sum(g) == target


def test_row_sums_at_the_tolerance(table, dev):
    """Sums 2 ulp above / 4 half-ulp below one pass the test, 3 ulp above / 5 half-ulp below fail it."""
    tr, plan, f = table
    up, down = np.spacing(1.0), np.spacing(1.0) / 2
    inside, outside = (1.0 + 2 * up, 1.0 - 4 * down), (1.0 + 3 * up, 1.0 - 5 * down)
    assert all(abs(x - 1.0) <= TOL for x in inside) and all(abs(x - 1.0) > TOL for x in outside)
    rng = np.random.default_rng(9)
    kind = rng.integers(0, 5, size=f.shape[0])       # 0: as it is, 1-2: inside, 3-4: outside
    g = f.copy()
    for k, target in enumerate(inside + outside, start=1):
        sel = np.flatnonzero(kind == k)
        rows, hit = _nudge(f[sel], target)
        assert hit.mean() > 0.9, (target, hit.mean())
        g[sel[hit]] = rows[hit]
    _check(tr, plan, g, dev, "tolerance")


@pytest.mark.parametrize("scaled", [False, True])
def test_dense_table(scaled, dev):
    """Rows of large totals: in-tile heavy rows (nrow = 255) and the global heavy lists beside the checked rows."""
    from bear_amd import kernels
    n = 200_000
    tr = kernels.synth_counts(3, 0, n, dev, dense=True, want=("train",))["train"]
    plan = kernels.Plan(tr, 5)
    f = kernels.synth_prior(3, 0, n, dev).cpu().numpy()
    if scaled:
        f = f * np.linspace(0.5, 2.0, n)[:, None]
    _check(tr, plan, f, dev, ("dense", scaled), normalized_too=not scaled)


_DET_SCRIPT = r"""
import json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from bear_amd import _lib, kernels
dev = torch.device("cuda", 0)
n = 2_000_000
tr = kernels.synth_counts(13, 0, n, dev, want=("train",))["train"]
plan = kernels.Plan(tr, 5)
f = kernels.synth_prior(13, 0, n, dev)
rows = torch.arange(0, n, 997, device=dev)
f[rows] *= 1.0005                                    # failing rows scattered over many tiles
runs = [kernels.dm_prior_planned(plan, f, -0.3).cpu().numpy().tobytes().hex() for _ in range(3)]
print("RESULT " + json.dumps({"det": bool(_lib.lib().bear_deterministic_build()), "runs": runs}))
"""


def test_deterministic_build_same_bits(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "det_rowsum.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    assert res["det"], res
    assert len(set(res["runs"])) == 1, res["runs"]
