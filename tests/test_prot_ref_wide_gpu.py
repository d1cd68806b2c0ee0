"""bear_ref's training step on the protein alphabet (rows of 21): dm_ref_wide_kernel (the stop net function) and
dm_refmix_wide_kernel (a net function with parameters; kernels_refmix_wide.h) against the width-generic oracle and, at W = 5,
against the trusted 5-wide entries; bear_ref.train on a protein table through them.

Tolerances (those test_prot_gpu.py holds dm_prior_wide to): sum LL 1e-11 relative; a scalar gradient within 2e-13 of its own L1
mass, the mass being sum |terms| of the oracle's formulas (dLdf df/dtau_s, dLdf df/dnu_s, g (-f / h)); gradient rows within
2e-13 sum |want|."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bear_oracle as o
from bear_amd import _lib, _train, ar_funcs, bear_ref, dataloader, kernels
from conftest import ROOT
from test_prot_cpu import make_prot_table, write_prot_tsv

pytestmark = pytest.mark.gpu
EPS = 1e-7
W = 21
POINTS = [(0.0, float(np.log(1 / 30)), float(-np.log(100))),       # where bear_ref starts
          (0.37, -1.2, -0.8)]                                       # ... and where the net weight matters
LL_RTOL, MASS_RTOL = 1e-11, 2e-13


def _dev_counts(c):
    return torch.from_numpy(np.array(c, dtype=np.uint32).view(np.int32)).cuda()


def keras_adam_np(p, g, m, v, t, lr=0.01, b1=0.9, b2=0.999, eps=1e-7):
    m[...] = b1 * m + (1 - b1) * g
    v[...] = b2 * v + (1 - b2) * g * g
    lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    p[...] = p - lr_t * m / (np.sqrt(v) + eps)


def _scalars(*vals):
    return [torch.tensor([float(v)], dtype=torch.float64, device="cuda") for v in vals]


@functools.lru_cache(maxsize=None)
def _tables():
    """name -> (train rows, reference rows); built once, never written to."""
    rng = np.random.default_rng(11)
    _, sparse = make_prot_table(seed=5, n=1037, num_ds=3)            # 1037: no multiple of either kernel's tile
    tr, rf = sparse[0], sparse[2]
    t = {"sparse": (tr, rf), "empty": (tr[:0], rf[:0])}
    for k in (1, 127, 128, 129, 255, 256, 257):                      # around the tiles of both kernels (128 and 256 contexts)
        t["first%d" % k] = (tr[:k], rf[:k])
    t["dense"] = (rng.integers(1000, 100_000, (700, W)).astype(np.uint32), rng.integers(1000, 100_000, (700, W)).astype(np.uint32))
    t["ref_zero"] = (tr, np.zeros_like(rf))                          # contexts the reference never saw: flat rows of eps
    stop_only = np.zeros_like(rf)
    stop_only[:, -1] = rng.integers(1, 500, len(rf))
    t["ref_stop_only"] = (tr, stop_only)                             # the stop column of the reference is ignored
    for a, b in t.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return t


TABLES = ["sparse", "first1", "first127", "first128", "first129", "first255", "first256", "first257", "empty", "dense", "ref_zero",
          "ref_stop_only"]


def _softmax_rows(rng, n, width, kind="softmax"):
    z = rng.normal(size=(n, width)) * 2.0
    g = np.exp(z - z.max(1, keepdims=True))
    g /= g.sum(1, keepdims=True)
    if kind == "tiny" and n:
        g[rng.random((n, width)) < 0.1] = 1e-300                     # entries near the bottom of the double range
    if kind == "scaled" and n:
        g = g * rng.uniform(0.5, 2.0, (n, 1))                        # rows that are not normalised
    return np.ascontiguousarray(g)


def _want(c, rf, point, train_ar, g=None):
    """o.bear_ref_step and the L1 masses of its three scalar gradients, from the oracle's own formulas."""
    h_s, tau_s, nu_s = point
    want = o.bear_ref_step(c, rf, h_s, tau_s, nu_s, train_ar=train_ar, net_probs=g)
    cf = np.asarray(c, dtype=np.float64)
    r = o.ref_input(rf, EPS)
    A = cf.shape[-1] - 1
    gn = np.broadcast_to(o.ar_func_stop(None, A) if g is None else g, cf.shape)
    nw, tau = np.exp(nu_s), np.exp(tau_s)
    E = np.exp(-tau)
    shape = np.r_[np.ones(A), 0.0]
    norm = r / r.sum(-1, keepdims=True)
    f = (nw * gn + (1.0 / A) * shape + E * (norm - (1.0 / A) * shape)) / (nw + 1.0)
    df_dtau_s = (-tau * E) * (norm - (1.0 / A) * shape) / (nw + 1.0)
    df_dnu_s = nw * (gn - f) / (nw + 1.0)
    if train_ar:
        dLdf, mass_h = cf / (f + EPS), 0.0
    else:
        h = np.exp(h_s)
        gc = o.dm_grad_concentration(f / h + EPS, cf)
        dLdf, mass_h = gc / h, np.abs(gc * (-f / h)).sum()
    return want, (mass_h, np.abs(dLdf * df_dtau_s).sum(), np.abs(dLdf * df_dnu_s).sum())


def _check_sums(got, want, mass, train_ar, what):
    print(what, "got", got.tolist(), "want", [want["ll"], want["d_h_signed"], want["d_tau_signed"], want["d_nu_signed"]], "mass", mass)
    assert np.isclose(got[0], want["ll"], rtol=LL_RTOL, atol=0), (what, got[0], want["ll"])
    if train_ar:
        assert got[1] == 0.0, what
    for k, name in ((1, "d_h_signed"), (2, "d_tau_signed"), (3, "d_nu_signed")):
        assert abs(got[k] - want[name]) <= MASS_RTOL * mass[k - 1], (what, name, got[k], want[name], mass[k - 1])


# ------------------------------------------------------------------ 1. the stop kernel against the oracle
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("train_ar", [False, True])
def test_dm_ref_wide_matches_oracle(table, train_ar):
    c, rf = _tables()[table]
    cd, rd = _dev_counts(c), _dev_counts(rf)
    for point in POINTS:
        got = kernels.dm_ref_wide(cd, rd, *point, train_ar=train_ar).cpu().numpy()
        if not len(c):
            assert got.tolist() == [0.0, 0.0, 0.0, 0.0]
            continue
        want, mass = _want(c, rf, point, train_ar)
        _check_sums(got, want, mass, train_ar, (table, train_ar, point))
    if table == "ref_stop_only":                 # ... ignored: the sums of the all-zero reference, bit for bit
        zero = kernels.dm_ref_wide(cd, _dev_counts(np.zeros_like(rf)), *POINTS[1], train_ar=train_ar)
        assert torch.equal(zero, kernels.dm_ref_wide(cd, rd, *POINTS[1], train_ar=train_ar))


# ------------------------------------------------------------------ 2. the ref-mix kernel against the oracle
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("train_ar", [False, True])
@pytest.mark.parametrize("rows", ["softmax", "tiny", "scaled"])
def test_dm_refmix_wide_matches_oracle(table, train_ar, rows):
    c, rf = _tables()[table]
    g = _softmax_rows(np.random.default_rng(len(c) + 3), len(c), W, rows)
    cd, rd, gd = _dev_counts(c), _dev_counts(rf), torch.from_numpy(g).cuda()
    for point in POINTS:
        out, grad = kernels.dm_refmix_wide_dev(cd, gd, rd, *_scalars(*point), train_ar=train_ar)
        got, grad = out.cpu().numpy(), grad.cpu().numpy()
        assert grad.shape == c.shape
        if not len(c):
            assert got.tolist() == [0.0, 0.0, 0.0, 0.0]
            continue
        want, mass = _want(c, rf, point, train_ar, g)
        _check_sums(got, want, mass, train_ar, (table, train_ar, rows, point))
        err, bound = np.abs(grad - want["d_net"]).max(), MASS_RTOL * np.abs(want["d_net"]).sum()
        print("rows: max err", err, "bound", bound)
        assert err <= bound
        assert (grad[c.sum(1) == 0] == 0).all()                      # contexts without training counts: exact zeros
    assert torch.equal(gd, torch.from_numpy(g).cuda())               # the net rows are read only


# ------------------------------------------------------------------ 3. width 5 against the 5-wide entries
@pytest.mark.parametrize("train_ar", [False, True])
def test_ref_wide_kernels_at_width_5_match_the_5_wide_entries(train_ar, ysd1):
    _, counts = ysd1
    c, rf = counts[:, 0].astype(np.uint32), counts[:, 1].astype(np.uint32)
    cd, rd = _dev_counts(c), _dev_counts(rf)
    for point in POINTS:
        ref = kernels.dm_ref(cd, rd, *point, train_ar=train_ar).cpu().numpy()
        got = kernels.dm_ref_wide(cd, rd, *point, train_ar=train_ar).cpu().numpy()
        print("stop", point, got.tolist(), ref.tolist())
        assert np.allclose(got, ref, rtol=1e-12, atol=0)
    g = _softmax_rows(np.random.default_rng(2), len(c), 5)
    gd = torch.from_numpy(g).cuda()
    ref_in = torch.from_numpy(o.ref_input(rf)).cuda()
    plan = kernels.Plan(cd, 5)
    for point in POINTS:
        sc = _scalars(*point)
        ref, gref = kernels.dm_refmix_planned_dev(plan, gd, ref_in, *sc, train_ar=train_ar)
        got, gg = kernels.dm_refmix_wide_dev(cd, gd, rd, *sc, train_ar=train_ar)
        ref, got, gw = ref.cpu().numpy(), got.cpu().numpy(), gref.cpu().numpy()
        print("mix", point, got.tolist(), ref.tolist())
        assert np.allclose(got, ref, rtol=1e-12, atol=0)
        assert np.allclose(gg.cpu().numpy(), gw, rtol=1e-12, atol=1e-13 * np.abs(gw).max())


# ------------------------------------------------------------------ 4. more tiles than blocks
@pytest.mark.parametrize("kernel", ["stop", "mix"])
def test_more_tiles_than_blocks(kernel):
    """A table of grid cap * tile + tile + 3 rows: every block takes a second tile, one a ragged third."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tile, per_cu = ((kernels.REF_WIDE_TILE[W], kernels.REF_WIDE_BLOCKS_PER_CU) if kernel == "stop"
                    else (kernels.REFMIX_WIDE_TILE[W], kernels.REFMIX_WIDE_BLOCKS_PER_CU))
    n = cus * per_cu * tile + tile + 3
    rng = np.random.default_rng(17)
    c = np.where(rng.random((n, W)) < 0.1, rng.poisson(6.0, (n, W)), 0).astype(np.uint32)
    rf = np.where(rng.random((n, W)) < 0.15, rng.poisson(9.0, (n, W)), 0).astype(np.uint32)
    cd, rd = _dev_counts(c), _dev_counts(rf)
    point = POINTS[1]
    for train_ar in (False, True):
        if kernel == "stop":
            want, mass = _want(c, rf, point, train_ar)
            got = kernels.dm_ref_wide(cd, rd, *point, train_ar=train_ar).cpu().numpy()
        else:
            g = _softmax_rows(np.random.default_rng(5), n, W)
            want, mass = _want(c, rf, point, train_ar, g)
            out, grad = kernels.dm_refmix_wide_dev(cd, torch.from_numpy(g).cuda(), rd, *_scalars(*point), train_ar=train_ar)
            got, grad = out.cpu().numpy(), grad.cpu().numpy()
            assert np.abs(grad - want["d_net"]).max() <= MASS_RTOL * np.abs(want["d_net"]).sum()
            assert (grad[c.sum(1) == 0] == 0).all()
        _check_sums(got, want, mass, train_ar, (kernel, n, train_ar))


# ------------------------------------------------------------------ 4b. the two kernels are one row body
@pytest.mark.parametrize("train_ar", [False, True])
@pytest.mark.parametrize("tiles", ["two_and_77", "more_than_blocks"])
def test_refmix_of_stop_rows_is_the_stop_kernel_byte_for_byte(train_ar, tiles):
    """rfw_row<W, AR, MIX> is the body of both kernels.  At width 5 both use tiles of 512 and three blocks per CU, so a context lands
    on the same thread of the same block in both; with net rows equal to the stop row (1.0 in the last column) the ref-mix kernel
    must leave the four sums of the stop kernel bit for bit.  Both read their parameters from device memory."""
    assert kernels.REF_WIDE_TILE[5] == kernels.REFMIX_WIDE_TILE[5] == 512
    assert kernels.REF_WIDE_BLOCKS_PER_CU == kernels.REFMIX_WIDE_BLOCKS_PER_CU
    cap = torch.cuda.get_device_properties(0).multi_processor_count * kernels.REF_WIDE_BLOCKS_PER_CU
    n = 2 * 512 + 77 if tiles == "two_and_77" else cap * 512 + 512 + 3
    rng = np.random.default_rng(23)
    c = np.where(rng.random((n, 5)) < 0.4, rng.poisson(6.0, (n, 5)), 0).astype(np.uint32)
    rf = np.where(rng.random((n, 5)) < 0.5, rng.poisson(9.0, (n, 5)), 0).astype(np.uint32)
    cd, rd = _dev_counts(c), _dev_counts(rf)
    g = torch.zeros((n, 5), dtype=torch.float64, device="cuda")
    g[:, 4] = 1.0
    for point in POINTS:
        theta = torch.tensor(point, dtype=torch.float64, device="cuda")
        stop = torch.full((4,), np.nan, dtype=torch.float64, device="cuda")
        kernels.ref_train_reduce_wide(cd, rd, theta, stop, train_ar=train_ar)
        mix, _ = kernels.dm_refmix_wide_dev(cd, g, rd, theta[0:1], theta[1:2], theta[2:3], train_ar=train_ar)
        stop, mix = stop.cpu().numpy(), mix.cpu().numpy()
        print(tiles, train_ar, point, "stop", stop.tolist(), "mix", mix.tolist())
        assert np.isfinite(stop).all() and stop[0] != 0.0
        assert stop.tobytes() == mix.tobytes()


# ------------------------------------------------------------------ 5. repeatability
_REPEAT = (
    "import numpy as np, torch\nfrom bear_amd import kernels\nfrom test_prot_cpu import make_prot_table\n"
    "_, c = make_prot_table(seed=2, n=20000, num_ds=2)\n"
    "cd, rd = (torch.from_numpy(x.view(np.int32)).cuda() for x in (c[0], c[1]))\n"
    "z = np.random.default_rng(0).random((20000, 21)); g = torch.from_numpy(z / z.sum(1, keepdims=True)).cuda()\n"
    "sc = [torch.tensor([v], dtype=torch.float64, device='cuda') for v in (0.2, -1.2, -0.8)]\n"
    "def run(ar):\n"
    "    a = kernels.dm_ref_wide(cd, rd, 0.2, -1.2, -0.8, train_ar=ar)\n"
    "    b, rows = kernels.dm_refmix_wide_dev(cd, g, rd, *sc, train_ar=ar)\n"
    "    return [x.cpu().numpy().tobytes() for x in (a, b, rows)]\n"
    "for ar in (False, True):\n"
    "    assert run(ar) == run(ar)\n")


def test_same_call_same_bytes():
    exec(compile(_REPEAT, "repeat", "exec"), {})


def test_deterministic_build_same_call_same_bytes(tmp_path):
    script = tmp_path / "det_ref_wide.py"
    script.write_text("import sys\nsys.path.insert(0, sys.argv[1])\nsys.path.insert(0, sys.argv[1] + '/tests')\n"
                      "from bear_amd import _lib\nassert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH\n"
                      + _REPEAT + "print('DET_REF_WIDE_OK')\n")
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "DET_REF_WIDE_OK" in p.stdout, p.stdout + p.stderr


# ------------------------------------------------------------------ 6., 7. bear_ref.train on a protein table
def _prot_data(tmp_path, n=600, batch=250, seed=0):
    kmers, counts = make_prot_table(seed=seed, n=n, num_ds=3)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    return dataloader.dataloader(str(path), "prot", batch, 3), kmers, counts


def _spy(monkeypatch, name, calls):
    real = getattr(kernels, name)

    def wrapper(*a, **kw):
        calls[name] = calls.get(name, 0) + 1
        return real(*a, **kw)
    monkeypatch.setattr(kernels, name, wrapper)


def test_bear_ref_train_prot_stop_takes_the_wide_step(tmp_path, monkeypatch):
    """The stop net function on a protein table: the device-resident loop on bear_ref_train_step_wide_f64, captured in a HIP graph;
    the replayed graph equals the eager loop bit for bit (the eager run is asked for with BEAR_AMD_GRAPH_MAX_ROWS=0 and
    BEAR_AMD_NO_GRAPH=1: this loop is run_device_steps itself, which reads the latter); BEAR_AMD_UNFUSED_MIX=1 runs the former
    path (torch mixing around dm_prior_wide) to the same losses."""
    data, kmers, _ = _prot_data(tmp_path)
    n, epochs = len(kmers), 8
    calls = {}
    for name in ("ref_train_step_wide", "ref_train_reduce_wide", "dm_prior_wide"):
        _spy(monkeypatch, name, calls)

    def run():
        losses = []
        params, _, _ = bear_ref.train(data.repeat(epochs), n, epochs, 0, 2, "prot", 4, ar_funcs.make_ar_func_stop, {}, 0.01, "Adam", False,
                                      loss_save=losses)
        return np.array(losses), np.array([p.item() for p in params])
    graph = run()
    assert _train.LAST_RUN["graph"] and len(graph[0]) == 24
    assert calls.get("ref_train_step_wide", 0) + calls.get("ref_train_reduce_wide", 0) > 0 and "dm_prior_wide" not in calls
    monkeypatch.setenv("BEAR_AMD_GRAPH_MAX_ROWS", "0")
    monkeypatch.setenv("BEAR_AMD_NO_GRAPH", "1")
    eager = run()
    assert not _train.LAST_RUN["graph"]
    monkeypatch.delenv("BEAR_AMD_GRAPH_MAX_ROWS")
    monkeypatch.delenv("BEAR_AMD_NO_GRAPH")
    assert graph[0].tobytes() == eager[0].tobytes() and graph[1].tobytes() == eager[1].tobytes()
    assert "dm_prior_wide" not in calls
    monkeypatch.setenv("BEAR_AMD_UNFUSED_MIX", "1")
    unfused = run()
    monkeypatch.delenv("BEAR_AMD_UNFUSED_MIX")
    assert calls.get("dm_prior_wide", 0) > 0
    print("max rel diff of the losses, fused / unfused:", np.abs(graph[0] / unfused[0] - 1).max())
    assert np.allclose(graph[0], unfused[0], rtol=1e-10, atol=0)


@pytest.mark.parametrize("train_ar", [False, True])
def test_bear_ref_train_prot_linear_matches_oracle_loop(train_ar, tmp_path, monkeypatch):
    data, kmers, counts = _prot_data(tmp_path)
    n, B, epochs, lag = len(kmers), 250, 8, 4
    make = ar_funcs.make_ar_func_linear
    torch.manual_seed(3)
    _, init = make(lag, 20)
    init_np = [x.detach().numpy().copy() for x in init]
    start = [np.array(0.1), np.array(np.log(1 / 30)), np.array(-np.log(100))]
    calls = {}
    for name in ("dm_refmix_wide_dev", "dm_prior_wide"):
        _spy(monkeypatch, name, calls)

    def run():
        losses = []
        params, _, _ = bear_ref.train(data.repeat(epochs), n, epochs, 0, 2, "prot", lag, make, {}, 0.01, "Adam", train_ar,
                                      params_restart=start + init_np, loss_save=losses)
        return np.array(losses), [p.detach().cpu().numpy().copy() for p in params]
    losses, params = run()
    assert calls.get("dm_refmix_wide_dev", 0) > 0 and "dm_prior_wide" not in calls
    # the CPU loop: torch-CPU rows, the oracle's step, d_net back through autograd, tf.keras Adam
    f_cpu, p_cpu = make(lag, 20)
    with torch.no_grad():
        for a, b in zip(p_cpu, init_np):
            a.copy_(torch.as_tensor(b))
    th = np.array([float(x) for x in start])
    m3, v3 = np.zeros(3), np.zeros(3)
    ms, vs = [np.zeros(x.shape) for x in p_cpu], [np.zeros(x.shape) for x in p_cpu]
    codes = torch.as_tensor(data.codes())
    want_loss, t = [], 0
    for _ in range(epochs):
        for a in range(0, n, B):
            b = min(a + B, n)
            for q in p_cpu:
                q.grad = None
            g = f_cpu(codes[a:b])
            r = o.bear_ref_step(counts[0, a:b], counts[2, a:b], *th, train_ar=train_ar, net_probs=g.detach().numpy())
            scale = -(n / (b - a))
            g.backward(torch.as_tensor(scale * r["d_net"]))
            want_loss.append(-scale * r["ll"])
            grad3 = scale * np.array([r["d_h_signed"], r["d_tau_signed"], r["d_nu_signed"]])
            t += 1
            if train_ar:
                keras_adam_np(th[1:], grad3[1:], m3[1:], v3[1:], t)
            else:
                keras_adam_np(th, grad3, m3, v3, t)
            for i, q in enumerate(p_cpu):
                keras_adam_np(q.detach().numpy(), q.grad.numpy(), ms[i], vs[i], t)
    assert len(losses) == len(want_loss) == 24
    print("max rel diff of the losses:", np.abs(losses / np.array(want_loss) - 1).max())
    assert np.allclose(losses, want_loss, rtol=1e-9, atol=0)
    assert np.allclose([float(x) for x in params[:3]], th, rtol=1e-6, atol=1e-8)
    for got, want in zip(params[3:], p_cpu):
        assert np.allclose(got, want.detach().numpy(), rtol=1e-6, atol=1e-8)
    monkeypatch.setenv("BEAR_AMD_UNFUSED_MIX", "1")
    unfused, _ = run()
    monkeypatch.delenv("BEAR_AMD_UNFUSED_MIX")
    assert calls.get("dm_prior_wide", 0) > 0
    assert np.allclose(losses, unfused, rtol=1e-10, atol=0)


# ------------------------------------------------------------------ 8. refusals through the raw ABI
def test_raw_abi_refusals():
    L = _lib.lib()
    assert L.bear_abi_version() == 12
    ws = kernels.default_workspace(torch.device("cuda", 0))
    p = kernels._ptr
    n = 8
    c21 = torch.zeros((n + 1, W), dtype=torch.int32, device="cuda")
    g21 = torch.ones((n + 1, W), dtype=torch.float64, device="cuda")
    c7 = torch.zeros((n, 7), dtype=torch.int32, device="cuda")
    g7 = torch.ones((n, 7), dtype=torch.float64, device="cuda")
    theta = torch.zeros(3, dtype=torch.float64, device="cuda")
    m, v, t = torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    h, tau, nw = _scalars(0.0, -1.0, -1.0)
    out = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.empty_like(g21)
    off4 = ctypes.c_void_p(c21.data_ptr() + 4)                       # a row pointer that is 4-byte, not 16-byte aligned

    def stop(tr, rf, rows, width, o_):
        return L.bear_dm_ref_wide_f64(ws.handle, tr, rf, rows, width, 0.0, -1.0, -1.0, EPS, 0, o_, None)

    def reduce_(tr, rf, rows, width, o_):
        return L.bear_ref_train_reduce_wide_f64(ws.handle, tr, rf, rows, width, p(theta), EPS, 0, o_, None)

    def step(tr, rf, rows, width, o_):
        return L.bear_ref_train_step_wide_f64(ws.handle, tr, rf, rows, width, p(theta), p(m), p(v), p(t), EPS, 0, 0.01, -1.0, o_, None, 0, None)

    def mix(tr, rf, rows, width, o_, net=None):
        return L.bear_dm_refmix_wide_grad_f64(ws.handle, tr, p(g21) if net is None else net, rf, rows, width, p(h), p(tau), p(nw), EPS, 0,
                                              o_, p(grad), None)
    for fn in (stop, reduce_, step, mix):
        assert fn(p(c7), p(c7), n, 7, p(out)) == -1, fn.__name__                    # width 7
        assert fn(p(c21), p(c21), n, W, None) == -1, fn.__name__                    # NULL out
        assert fn(off4, p(c21), n, W, p(out)) == -1, fn.__name__                    # misaligned rows
        assert fn(p(c21), off4, n, W, p(out)) == -1, fn.__name__
    assert mix(p(c7), p(c7), n, 7, p(out), net=p(g7)) == -1
    assert mix(p(c21), p(c21), n, W, p(out), net=ctypes.c_void_p(g21.data_ptr() + 8)) == -1
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 4 and theta.tolist() == [0.0] * 3 and t.item() == 0.0     # nothing was launched
    for fn in (stop, reduce_, mix, step):                                           # n_rows = 0: zero sums
        out.fill_(7.0)
        assert fn(None, None, 0, W, p(out)) == 0, fn.__name__
        torch.cuda.synchronize()
        assert out.tolist() == [0.0] * 4, fn.__name__
    assert theta.tolist() == [0.0] * 3 and t.item() == 1.0           # (the step's update ran, on zero gradients)
    with pytest.raises(ValueError):
        kernels.dm_ref_wide(c7, c7, 0.0, -1.0, -1.0)
