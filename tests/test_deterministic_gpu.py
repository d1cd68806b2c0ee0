"""BEAR_AMD_DETERMINISTIC=1: parameter gradients that are bit-identical from run to run (SURVEY section 5 asked for the option;
include/bear_hip.h says what it does).  Linear step: fixed-point gradient tables -- d/d mat is also identical for any sharding of
the batch that uses the same bound.  Convolutional step: one wave per block."""
import math
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from test_parity_gpu import CASES_REF, ELBO_RTOL, _close, _linear_oracle, _mass_close, _sorted_by_kmer, _to_dev

pytestmark = pytest.mark.gpu


def _sorted_table(n, lag, dev, seed=5, fixed=0):
    import torch
    from bear_amd import kernels
    t = kernels.synth_counts(20211012, 0, n, dev, want=("train",))["train"]
    gen = torch.Generator(dev).manual_seed(seed)
    codes = torch.randint(0, 4, (n, lag), dtype=torch.int8, device=dev, generator=gen)
    codes[:, :fixed] = 1             # (a table dense in k-mer space: prefixes repeat)
    key = torch.zeros(n, dtype=torch.int64, device=dev)
    for l in range(lag):
        key = key * 6 + codes[:, l].to(torch.int64)
    codes = codes[torch.argsort(key)].contiguous()
    return t, codes


@pytest.mark.parametrize("train_ar", [False, True])
def test_linear_step_is_bit_reproducible_and_shard_invariant(train_ar, monkeypatch):
    import torch
    from bear_amd import kernels
    dev = torch.device("cuda", 0)
    n, lag = 3_000_000, 13
    t, codes = _sorted_table(n, lag, dev)
    idx = kernels.linear_index(kernels.pack_kmers(codes), lag)
    mat = 0.3 * torch.randn(lag, 5, 5, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(3))
    plan = kernels.Plan(t, 5)
    total, bound = plan.count_total()
    assert total == [float(t.to(torch.int64).sum()), float((t != 0).sum()), float(t.max())] and bound == total
    monkeypatch.delenv("BEAR_AMD_DETERMINISTIC", raising=False)
    ref_out, ref_g = (x.clone() for x in kernels.dm_linear(plan, idx, mat, -0.2, train_ar=train_ar))
    monkeypatch.setenv("BEAR_AMD_DETERMINISTIC", "1")
    runs = []
    for paired in (False, True):
        if paired:
            assert plan.pair_contexts(idx, lag)
        for _ in range(3):
            o, g = kernels.dm_linear(plan, idx, mat, -0.2, train_ar=train_ar)
            runs.append((o.clone(), g.clone()))
    for o, g in runs:
        assert torch.equal(g, runs[0][1])                    # plain and paired lists, every run: the same bits
        assert torch.allclose(o, ref_out, rtol=1e-13, atol=0)
    scale = float(ref_g.abs().max())
    # one rounding to bound 2^-62 per context and letter: far below the rounding of the fp64 sums it is compared with
    assert float((runs[0][1] - ref_g).abs().max()) <= 1e-12 * scale
    assert float(runs[0][1].sum(-1).abs().max()) <= 1e-9 * scale       # a softmax gradient sums to zero over the letters
    # the same batch cut into 2 / 4 / 7 row shards (ragged), every shard on the batch's bound: the shards' INTEGER sums add up to
    # the batch's exactly; each becomes a double on its own (one rounding each), so the doubles agree to the last bits
    for pieces in (2, 4, 7):
        cuts = [0] + [int(n * (k + 1) / pieces) // 4 * 4 + (3 if k == 0 else 0) for k in range(pieces - 1)] + [n]
        tot = torch.zeros_like(ref_g)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ts, ix = t[lo:hi].clone(), idx[lo:hi].clone()        # (fresh, 16-byte aligned buffers)
            ps = kernels.Plan(ts, 5)
            ps.set_count_bound(total)
            if pieces != 4:                                       # paired and plain shards mixed: the same integers either way
                ps.pair_contexts(ix, lag)
            tot += kernels.dm_linear(ps, ix, mat, -0.2, train_ar=train_ar)[1]
        assert float((tot - runs[0][1]).abs().max()) <= 4e-15 * scale, pieces
    with pytest.raises(Exception):
        plan.set_count_bound([total[0] / 2, total[1], total[2]])    # a bound below the plan's own total is refused


def test_linear_step_default_mode_unchanged(monkeypatch):
    """Without the switch the tables hold doubles (LDS floating-point atomics): results agree with the deterministic ones to
    rounding, and the switch is read per call."""
    import torch
    from bear_amd import kernels
    dev = torch.device("cuda", 0)
    n, lag = 400_000, 9
    t, codes = _sorted_table(n, lag, dev, seed=9)
    idx = kernels.linear_index(kernels.pack_kmers(codes), lag)
    mat = 0.1 * torch.randn(lag, 5, 5, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(4))
    plan = kernels.Plan(t, 5)
    monkeypatch.setenv("BEAR_AMD_DETERMINISTIC", "1")
    _, g1 = (x.clone() for x in kernels.dm_linear(plan, idx, mat, 0.1))
    monkeypatch.setenv("BEAR_AMD_DETERMINISTIC", "0")
    _, g0 = (x.clone() for x in kernels.dm_linear(plan, idx, mat, 0.1))
    assert float((g1 - g0).abs().max()) <= 1e-12 * float(g0.abs().max())


def test_cnn_step_is_bit_reproducible(monkeypatch):
    import torch
    from bear_amd import ar_funcs, kernels
    dev = torch.device("cuda", 0)
    n, lag, fw = 300_000, 13, 8
    t, codes = _sorted_table(n, lag, dev, seed=7, fixed=4)
    keep = (t != 0).any(dim=1).nonzero().squeeze(1)
    t, codes = t.index_select(0, keep).contiguous(), codes.index_select(0, keep).contiguous()
    n = t.shape[0]
    packed = kernels.pack_kmers(codes)
    _, params = ar_funcs.make_ar_func_cnn(lag, 4, filter_width=fw, device=dev, generator=torch.Generator(dev).manual_seed(10))
    theta = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev)] + [q.detach().reshape(-1) for q in params]).contiguous()
    plan = kernels.Plan(t, 5)
    monkeypatch.delenv("BEAR_AMD_DETERMINISTIC", raising=False)
    bufs = kernels.cnn_step_buffers(n, lag, fw, dev, ws=plan.ws)
    pk = torch.zeros(theta.numel() + 1, dtype=torch.float64, device=dev)
    kernels.net_cnn_train_reduce(plan, packed, lag, fw, theta, bufs, pk)
    ref = pk.clone()
    for levels in (False, True):
        if levels:
            assert plan.attach_cnn_levels(packed, lag, fw) >= 1
        monkeypatch.setenv("BEAR_AMD_DETERMINISTIC", "1")
        outs = []
        for _ in range(3):
            pk.zero_()
            kernels.net_cnn_train_reduce(plan, packed, lag, fw, theta, bufs, pk)
            outs.append(pk.clone())
        # the parameter gradients [2:] (sum LL and d/dh follow the draw of the work units in this library: the deterministic
        # build fixes those too, test_deterministic_build_whole_trajectory)
        assert torch.equal(outs[0][2:], outs[1][2:]) and torch.equal(outs[0][2:], outs[2][2:]), levels
        assert abs(float(outs[0][0] - ref[0])) <= 1e-12 * abs(float(ref[0]))
        assert float((outs[0][1:] - ref[1:]).abs().max()) <= 1e-10 * float(ref[1:].abs().max())
        monkeypatch.delenv("BEAR_AMD_DETERMINISTIC", raising=False)


def _fx_unit(bound, h_s, train_ar):
    """The rounding unit of the fixed-point tables as include/bear_hip.h and lin_fx_scale state it: bound = the sum of all counts,
    in BEAR mode also cells (1 + u (1 + ln c_max)) with u = 1 / exp(h_s), at least 1; unit = 2^(e - 62) with bound < 2^e."""
    counts, cells, cmax = bound
    b = counts
    if not train_ar:
        u = 1.0 / math.exp(h_s)
        b = min(b, cells * (1.0 + u * (1.0 + math.log(max(cmax, 1.0)))))
    b = max(b, 1.0)
    e = math.frexp(b)[1]
    return math.ldexp(1.0, e - 62), b


def _run_codes(n, lag, rng):
    """Contexts as in test_fused_linear_head_paired_contexts: few distinct prefixes (runs of many contexts) for most rows, random
    contexts for the rest, one row in fifty with a start symbol or an unknown letter."""
    n_pre = max(1, n // 40)
    pre = rng.integers(0, 4, size=(n_pre, max(lag - 3, 0))).astype(np.int8)
    codes = rng.integers(0, 4, size=(n, lag)).astype(np.int8)
    half = n - n // 33
    codes[:half, :max(lag - 3, 0)] = pre[rng.integers(0, n_pre, size=half)]
    for r in rng.choice(n, size=max(2, n // 50), replace=False):
        codes[r, rng.integers(0, lag)] = 4 if rng.random() < 0.6 else -1
    return codes


# DESIGN 4.11's figure for the rounding unit, in the form "all 2 cells conversions that can reach one entry round the same way"
# against the oracle's largest gradient (no kernel output enters it).  1e-12 holds on `edge` (largest value 2.9e-13, lag 5 at
# h_s = -2.5); on `dense` it holds for h_s >= 1.5 and in the multinomial (<= 4.7e-13) but not under a small h, where the cells
# bound grows with u = 1 / h while the gradients do not: 1.8e-12 at h_s = 0, 1.5e-11 at h_s = -2.5 (lag 9).  ONE conversion is
# below 5e-16 of the largest gradient on both tables.
FX_WORST_CASE = {"edge": 1e-12, "dense": 2e-11}
FX_PARAMS = [(-2.5, False), (0.0, False), (1.5, False), (8.0, False), (0.3, True)]


@pytest.mark.parametrize("lag", [5, 13, 14, 9])            # 2, 6, 7 letter groups as compile-time constants, and the run-time form
@pytest.mark.parametrize("case", ["sparse", "dense", "edge", "ysd1", "mixed_heavy"])
def test_fixed_point_linear_step_matches_oracle(case, lag, ysd1, monkeypatch):
    """dm_linear_plan_kernel<AR, PAIRED, DET = true, NGK> against the oracle chain -- every instantiation launch_linear can choose:
    AR x paired x NGK in {2, 6, 7, 0} -- on tables whose large-count cells overflow to the plan's global lists (dense, edge,
    mixed_heavy: the overflow-item loop under DET) and under an h large enough that the cells bound of lin_fx_scale binds."""
    import torch
    from bear_amd import kernels
    dev = torch.device("cuda", 0)
    tr = ysd1[1][:, 0].astype(np.uint32) if case == "ysd1" else CASES_REF[case]()[0]
    n = len(tr)
    rng = np.random.default_rng(lag * 13 + n)
    codes = _run_codes(n, lag, rng)
    order = _sorted_by_kmer(codes)
    codes, tr = codes[order], np.ascontiguousarray(tr[order])
    mat = rng.normal(size=(lag, 5, 5)) * 0.4
    d_mat = torch.from_numpy(mat).to(dev)
    plan = kernels.Plan(_to_dev(tr, dev), 5)
    idx = kernels.linear_index(kernels.pack_kmers(torch.from_numpy(codes).to(dev)), lag)
    total, bound = plan.count_total()
    assert bound == total == [float(tr.sum(dtype=np.uint64)), float((tr != 0).sum()), float(tr.max())]
    cells = bound[1]
    oracle = [_linear_oracle(tr, codes, mat, h_s, ar) for h_s, ar in FX_PARAMS]
    first = {}
    for paired in (False, True):
        if paired:
            assert plan.pair_contexts(idx, lag) is True and plan.pair_info()[0] >= 1
        for (h_s, ar), (want, wantg) in zip(FX_PARAMS, oracle):
            what = (case, lag, paired, h_s, ar)
            unit, b = _fx_unit(bound, h_s, ar)
            gmax = np.abs(wantg).max()
            monkeypatch.setenv("BEAR_AMD_DETERMINISTIC", "1")
            got, g = (x.clone() for x in kernels.dm_linear(plan, idx, d_mat, h_s, train_ar=ar))
            got2, g2 = (x.clone() for x in kernels.dm_linear(plan, idx, d_mat, h_s, train_ar=ar))
            monkeypatch.delenv("BEAR_AMD_DETERMINISTIC")
            _, g_fp = (x.clone() for x in kernels.dm_linear(plan, idx, d_mat, h_s, train_ar=ar))
            assert torch.equal(g, g2), what                                    # two launches: the same bits
            assert torch.equal(g, first.setdefault((h_s, ar), g)), what        # plain and paired lists: the same integers
            got, g, g_fp = got.cpu().numpy(), g.cpu().numpy(), g_fp.cpu().numpy()
            diff = np.abs(g - g_fp).max()
            print("fixed point %s: bound %.6g unit %.3g cells %d max|g| %.6g |det - fp| %.3g (allowed %.3g) unit*2*cells/max|g| %.3g"
                  % (what, b, unit, cells, gmax, diff, 0.5 * unit * 2 * cells + 1e-12 * gmax, unit * 2 * cells / gmax))
            _close(got[0], want[0], ELBO_RTOL)
            _mass_close(got[1], want[1], want[2], what)
            assert np.allclose(g, wantg, rtol=1e-9, atol=1e-9 * gmax), (what, np.abs(g - wantg).max())
            # one conversion (rounded to unit / 2) per context with counts and per overflow item: at most 2 cells of them reach an entry
            assert diff <= 0.5 * unit * 2 * cells + 1e-12 * gmax, (what, diff)
            if case in FX_WORST_CASE:                                          # the rounding unit against the gradient
                assert unit <= 1e-15 * gmax, (what, unit, gmax)
                assert unit * 2 * cells <= FX_WORST_CASE[case] * gmax, (what, unit, cells, gmax)


@pytest.mark.parametrize("mode", ["ar", "bear_h-30", "bear_h0"])
@pytest.mark.parametrize("c", [2 ** 30, 2 ** 30 - 1])
def test_fixed_point_sums_that_reach_the_bound(c, mode, monkeypatch):
    """The smallest case in which a wrong scale would wrap the 64-bit table: 1024 contexts of one 13-mer with all counts in letter
    0, a prior that leaves f_0 ~ 1e-6 -- every g of a table entry has the same sign and their sum comes close to the bound (in the
    multinomial w_0 = c f_0 / (f_0 + eps)); c = 2^30 makes the count sum exactly 2^40, where the scale's exponent steps up."""
    import torch
    from bear_amd import kernels
    dev = torch.device("cuda", 0)
    n, lag = 1024, 13
    monkeypatch.setenv("BEAR_AMD_DETERMINISTIC", "1")
    tr = np.zeros((n, 5), np.uint32)
    tr[:, 0] = c
    codes = np.tile(np.array([2, 0, 3, 1, 1, 0, 2, 3, 3, 1, 0, 2, 1], np.int8), (n, 1))
    mat = np.zeros((lag, 5, 5))
    mat[4, 1, 3] = math.log(1e6)                  # logits (0, 0, 0, ln 1e6, 0): f_3 ~ 1, the others ~ 1e-6
    ar, h_s = {"ar": (True, 0.3), "bear_h-30": (False, -30.0), "bear_h0": (False, 0.0)}[mode]
    want, wantg = _linear_oracle(tr, codes, mat, h_s, ar)
    plan = kernels.Plan(_to_dev(tr, dev), 5)
    total, bound = plan.count_total()
    assert bound == total == [float(n * c), float(n), float(c)]
    unit, b = _fx_unit(bound, h_s, ar)
    idx = kernels.linear_index(kernels.pack_kmers(torch.from_numpy(codes).to(dev)), lag)
    d_mat = torch.from_numpy(mat).to(dev)
    got, g = (x.clone() for x in kernels.dm_linear(plan, idx, d_mat, h_s, train_ar=ar))
    assert plan.pair_contexts(idx, lag) is True
    got_p, g_p = (x.clone() for x in kernels.dm_linear(plan, idx, d_mat, h_s, train_ar=ar))
    gmax = np.abs(wantg).max()
    print("reach the bound (%s, c = %d): bound %.6g = 2^%.3f, unit %.3g, largest |sum of g| %.6g = %.3g of the bound"
          % (mode, c, b, math.log2(b), unit, gmax, gmax / b))
    assert np.allclose(g.cpu().numpy(), wantg, rtol=1e-9, atol=1e-9 * gmax), (mode, c, np.abs(g.cpu().numpy() - wantg).max())
    # (sum LL is not compared here: with counts of 2^30 it is what 1024 terms of 2e10 leave of each other, below their rounding)
    assert torch.equal(g, g_p)                    # plain and paired lists: the same integers


def test_count_bound_limits(monkeypatch):
    """bear_plan_set_count_bound: a first component of 2^50 is refused, 2^50 - 1 is taken -- the unit is then bound 2^-62 of THAT
    bound, the gradient within one rounding per conversion of the floating-point launch, and repeats bit for bit; an all-zero table
    (bound 0: the floating-point kernel) gives an exactly zero gradient."""
    import torch
    from bear_amd import _lib, kernels
    dev = torch.device("cuda", 0)
    lag = 13
    tr = CASES_REF["sparse"]()[0]
    n = len(tr)
    rng = np.random.default_rng(50)
    codes = rng.integers(0, 4, size=(n, lag)).astype(np.int8)
    idx = kernels.linear_index(kernels.pack_kmers(torch.from_numpy(codes).to(dev)), lag)
    d_mat = torch.from_numpy(rng.normal(size=(lag, 5, 5)) * 0.4).to(dev)
    plan = kernels.Plan(_to_dev(tr, dev), 5)
    total, _ = plan.count_total()
    with pytest.raises(_lib.BearError):
        plan.set_count_bound([2.0 ** 50, total[1], total[2]])
    assert plan.count_total()[1] == total                     # (a refused bound leaves the plan as it was)
    plan.set_count_bound([2.0 ** 50 - 1, total[1], total[2]])
    bound = plan.count_total()[1]
    assert bound == [2.0 ** 50 - 1, total[1], total[2]]
    for h_s, ar in [(0.3, True), (0.0, False)]:
        unit, b = _fx_unit(bound, h_s, ar)
        assert unit == 2.0 ** -12 or not ar                   # multinomial: the count sum is the bound, 2^49 <= bound < 2^50
        monkeypatch.delenv("BEAR_AMD_DETERMINISTIC", raising=False)
        _, g_fp = (x.clone() for x in kernels.dm_linear(plan, idx, d_mat, h_s, train_ar=ar))
        monkeypatch.setenv("BEAR_AMD_DETERMINISTIC", "1")
        _, g1 = (x.clone() for x in kernels.dm_linear(plan, idx, d_mat, h_s, train_ar=ar))
        _, g2 = (x.clone() for x in kernels.dm_linear(plan, idx, d_mat, h_s, train_ar=ar))
        diff = float((g1 - g_fp).abs().max())
        print("count bound 2^50 - 1 (ar = %s): unit %.3g, |det - fp| %.3g, allowed %.3g" % (ar, unit, diff, 0.5 * unit * 2 * bound[1]))
        assert torch.equal(g1, g2)
        assert diff <= 0.5 * unit * 2 * bound[1], (ar, diff, unit)
    zero = kernels.Plan(torch.zeros((n, 5), dtype=torch.int32, device=dev), 5)
    assert zero.count_total() == ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    for ar in (False, True):
        out, g = kernels.dm_linear(zero, idx, d_mat, 0.2, train_ar=ar)
        assert torch.equal(g, torch.zeros_like(g)) and bool(torch.isfinite(out).all()), ar


_DET_SCRIPT = r"""
import hashlib, json, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from bear_amd import _lib, ar_funcs, bear_net, bear_ref, dataloader, kernels
assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH
dev = torch.device("cuda", 0)
out = {}
# kernel level: every step kernel three times, whole outputs
n = 700_000
t = kernels.synth_counts(20211012, 0, n, dev, want=("train", "ref"))
prior = kernels.synth_prior(20211012, 0, n, dev)
plan5, plan4 = kernels.Plan(t["train"], 5), kernels.Plan(t["train"], 4, ref=t["ref"])
def rep(name, fn):
    a = [fn() for _ in range(3)]
    flat = [torch.cat([x.reshape(-1).double() for x in (r if isinstance(r, (tuple, list)) else (r,)) if x is not None]) for r in a]
    out[name] = bool(torch.equal(flat[0], flat[1]) and torch.equal(flat[0], flat[2]))
rep("mode_N", lambda: kernels.dm_prior_planned(plan5, prior, -0.3).clone())
rep("mode_N_grad_rows", lambda: tuple(x.clone() for x in kernels.dm_prior_planned(plan5, prior, -0.3, want_grad=True)))
rep("mode_N_grad_rows_normalized", lambda: tuple(x.clone() for x in kernels.dm_prior_planned(plan5, prior, -0.3, want_grad=True, normalized=True)))
rep("mode_R", lambda: kernels.dm_ref_planned(plan4, t["ref"], 0.1, -3.4, -4.6).clone())
rep("mode_R_streaming", lambda: kernels.dm_ref_planned(kernels.Plan(t["train"], 4), t["ref"], 0.1, -3.4, -4.6).clone())
# the drivers: the bundled ysd1 table, 300 optimizer steps, twice; linear, cnn, reference
path = os.path.join(sys.argv[1], "bear_amd", "data", "ysd1_lag_5_file_0_preshuf.tsv")
data = dataloader.dataloader(path, "dna", 1500, 3)
def digest(params, h):
    m = hashlib.sha256()
    for p in list(params) + [h]:
        m.update(p.detach().cpu().numpy().tobytes())
    return m.hexdigest()
for name, mod, make, kw, extra in (("linear", bear_net, ar_funcs.make_ar_func_linear, {}, ()),
                                   ("cnn", bear_net, ar_funcs.make_ar_func_cnn, {"filter_width": 3}, ()),
                                   ("ref_stop", bear_ref, ar_funcs.make_ar_func_stop, {}, (2,))):
    ds = []
    for _ in range(2):
        torch.manual_seed(10)
        params, h, _ = mod.train(data.repeat(300), 1365, 300, 0, *extra, "dna", 5, make, kw, 0.01, "Adam", False)
        ds.append(digest(params, h))
    out["train_" + name] = ds[0] == ds[1]
    if name != "cnn":
        # ... and the ONE-launch optimizer step (the reduce kernel's last block runs Adam: what the two runs above took) ends in the
        # same bits as reduce + bear_train_apply_f64 in two launches
        from bear_amd import _train
        out["one_launch_" + name] = bool(_train.LAST_RUN.get("one_launch_steps"))
        os.environ["BEAR_AMD_TWO_LAUNCH_STEP"] = "1"
        torch.manual_seed(10)
        params, h, _ = mod.train(data.repeat(300), 1365, 300, 0, *extra, "dna", 5, make, kw, 0.01, "Adam", False)
        del os.environ["BEAR_AMD_TWO_LAUNCH_STEP"]
        out["two_launch_" + name] = not _train.LAST_RUN.get("one_launch_steps")
        out["one_launch_equals_two_launch_" + name] = digest(params, h) == ds[0]
print("RESULT " + json.dumps(out))
"""


def test_deterministic_build_whole_trajectory(tmp_path):
    """BEAR_AMD_DETERMINISTIC=1 at import loads libbear_hip_det.so (work units dealt statically): every output of every step kernel
    is bit-identical from launch to launch, and a 300-step training run of each driver ends in the same bits twice."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "det_run.py"
    script.write_text(_DET_SCRIPT)
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    assert res and all(res.values()), res


# The oracle parity tests that walk plans, item units and gradient tables, by family; (node ids, -k expression, cases).  The
# number of cases is counted by hand from the parametrisations: a selection cannot pass by being empty or by losing a case --
# update it only together with them.  A child costs ~4 s before its first test (interpreter, torch, the library, collection:
# profiles/det_parity_times.txt), so the families leave out their largest table, `sparse` (10 006 / 20 011 rows; the regular
# library's suite runs it); `mixed_heavy`, `edge` and `dense` stay in every family.
_NO_SPARSE = "not (sparse] or sparse-)"
_PAR, _DET, _MIX, _TRN, _CNN = ("tests/test_parity_gpu.py", "tests/test_deterministic_gpu.py", "tests/test_refmix_plan_gpu.py",
                                "tests/test_train_gpu.py", "tests/test_cnn_gpu.py")
DET_FAMILIES = {
    # 6 + 6 + 6 + 1 + 8 x 2 + 1
    "dm_plans": ([_PAR + "::test_planned_kernels_parity", _PAR + "::test_planned_ar_mode_parity", _PAR + "::test_dense_form_of_the_plan",
                  _PAR + "::test_planned_randomized_shapes", _PAR + "::test_reference_aware_plan_parity",
                  _PAR + "::test_mixed_heavy_reaches_the_caps"], _NO_SPARSE, 36),
    # 5 x 3 + 3 x 8 + 1 + 4 x 4 + 2 x 3 (the library is always fixed-point: the switch the last two set changes nothing here)
    "linear": ([_PAR + "::test_fused_linear_head_parity", _PAR + "::test_fused_linear_head_paired_contexts",
                _PAR + "::test_fused_linear_head_saturated_logits", _DET + "::test_fixed_point_linear_step_matches_oracle",
                _DET + "::test_fixed_point_sums_that_reach_the_bound"], _NO_SPARSE, 62),
    # 6 + 1 + 6 x 2 + 1
    "eval_mix": ([_PAR + "::test_eval_plan_kernel_parity", _PAR + "::test_eval_plan_many_models_and_zero_rows",
                  _MIX + "::test_refmix_plan_matches_the_oracle_chain_and_the_unfused_launches",
                  _MIX + "::test_refmix_plan_rows_without_counts_and_ragged_tiles"], _NO_SPARSE, 20),
    # 2 + 5 + 2 x 2 + 3 x 2 (the convolutional backward pass at its three smallest shapes, both forms)
    "train": ([_TRN + "::test_bear_ref_train_matches_oracle_loop", _TRN + "::test_bear_net_train_matches_oracle_loop",
               _TRN + "::test_one_launch_step_matches_the_two_launch_step", _CNN + "::test_cnn_backward_matches_torch_autograd"],
              "not test_cnn_backward_matches_torch_autograd or 2-1-3- or 13-8-31- or 13-8-33-", 17),
}


@pytest.mark.parametrize("family", list(DET_FAMILIES))
def test_det_library_parity(family):
    """libbear_hip_det.so against the ORACLE, not only against itself: the parity tests of one kernel family, unchanged, in a fresh
    process that loads the deterministic build -- its block-wide scan for the in-tile lists, the bitonic sort of a tile's items,
    the statically dealt work units, the merge-sorted global lists and reference buckets.  (A deterministic builder that drops an
    item gives the same wrong bits every run: the repeatability tests cannot see it.)"""
    ids, expr, cases = DET_FAMILIES[family]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    cmd = [sys.executable, os.path.join(root, "tests", "det_parity_worker.py")] + [os.path.join(root, i) for i in ids]
    if expr:
        cmd += ["-k", expr]
    t0 = time.perf_counter()
    p = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    print("det parity %s: %.1f s" % (family, time.perf_counter() - t0))
    tail = p.stdout[-4000:] + p.stderr[-2000:]
    assert p.returncode == 0, tail
    assert any(ln.startswith("DET_LIBRARY ") and ln.endswith("libbear_hip_det.so") for ln in p.stdout.splitlines()), tail
    summary = [ln for ln in p.stdout.splitlines() if re.search(r"\d+ passed", ln)][-1]
    n = {k.rstrip("s"): int(v) for v, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed)", summary)}
    assert n.get("failed", 0) == 0 and n.get("skipped", 0) == 0 and n.get("error", 0) == 0 and n.get("xfailed", 0) == 0, summary
    assert n["passed"] == cases, (summary, cases)
