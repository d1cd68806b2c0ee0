"""GPU tests of bear_net's linear step at the protein alphabet's width as one launch (bear_dm_linear_wide_f64,
bear_net_linear_train_{reduce,step}_wide_f64; kernels_linear_wide.h): the primitive against the oracle (ar_func_linear on a one-hot,
bear_net_step, the NumPy chain of the softmax backward and the einsum's transpose) and against the three launches it replaces, equal
bytes from call to call and in the deterministic build, the reduce and step forms, the raw ABI's refusals, and bear_net.train on a
protein table -- alone, against the unfused path, against a NumPy loop, and on two ranks."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bear_oracle as o
import c_oracle as co
from bear_amd import _lib, _train, ar_funcs, bear_net, dataloader, kernels, summarize
from conftest import ROOT
from test_dist_gpu import _launch
from test_prot_cpu import make_prot_table, write_prot_tsv
from test_prot_gpu import keras_adam_np
from test_prot_linear_rows_gpu import _codes, _onehot

pytestmark = pytest.mark.gpu

W = 21
EPS = 1e-7
MAX_LAG = kernels.LINEAR_WIDE_MAX_LAG
TILE = kernels.LINEAR_STEP_WIDE_TILE
GRAD_RTOL = 1e-11        # of the largest entry of d/d mat: the row kernels' bound (test_prot_linear_rows_gpu.py)
CELL_RTOL = 1e-12        # of a gradient-row cell's own mass: the bound test_prot_gpu.py holds gradient rows to
GRID_CAP = "more tiles than the capped grid has blocks: a block takes more than one"
EMPTY = 0
SHAPES = [(1, 1), (1, 70), (2, 64), (3, 127), (3, 128), (3, 129), (5, 1365), (12, 4097), (MAX_LAG, 257), (3, GRID_CAP), (4, EMPTY)]
H_SIGNED = [-3.0, 0.0, 2.0]


def _shape_id(v):
    return "cap" if v is GRID_CAP else str(v)


def _n(n):
    if n is GRID_CAP:       # two blocks per CU, each with a tile of its own, and then some: partial last tile
        return torch.cuda.get_device_properties(0).multi_processor_count * kernels.LINEAR_STEP_WIDE_BLOCKS_PER_CU * TILE + 5 * TILE + 77
    return n


def _counts(n, rng):
    """make_prot_table's recipe (Poisson counts on ~15 % of the cells, a rate per row), then: a handful of counts beyond the product
    path (up to 3e5), rows with one non-zero cell, rows with all 21, and ~30 % rows without any count."""
    mask = rng.random((n, W)) < 0.15
    c = np.where(mask, rng.poisson(rng.uniform(0.5, 40.0, (n, 1)), (n, W)), 0).astype(np.uint32)
    if n:
        big = rng.choice(n, min(6, n), replace=False)
        c[big, rng.integers(0, W, big.size)] = rng.integers(100_000, 300_001, big.size)
        kind = rng.random(n)
        one = np.nonzero((kind >= 0.30) & (kind < 0.36))[0]
        c[one] = 0
        c[one, rng.integers(0, W, one.size)] = rng.integers(1, 50, one.size)
        full = np.nonzero((kind >= 0.36) & (kind < 0.40))[0]
        c[full] = rng.integers(1, 30, (full.size, W))
        c[kind < 0.30] = 0
    return np.ascontiguousarray(c)


@functools.lru_cache(maxsize=None)
def _inputs(lag, n):
    """One seeded problem per shape, shared by the tests (read-only): codes, counts, mat, the one-hot and the oracle's rows."""
    n = _n(n)
    rng = np.random.default_rng(lag * 1000 + n)
    codes = _codes(n, lag, rng)
    counts = _counts(n, rng)
    mat = rng.normal(size=(lag, W, W)) * 0.4
    oh = _onehot(codes)
    f = o.ar_func_linear(oh, mat) if n else np.zeros((0, W))
    for a in (codes, counts, mat, oh, f):
        a.setflags(write=False)
    return codes, counts, mat, oh, f


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


def _dev_counts(c):
    return torch.from_numpy(np.array(c, dtype=np.uint32).view(np.int32)).cuda()


def _chain(oh, f, q):
    """d / d mat from the rows' gradient q: softmax backward, then the transpose of the einsum of ar_func_linear."""
    return np.einsum("njk,nl->jkl", oh, f * (q - (f * q).sum(-1, keepdims=True)))


@functools.lru_cache(maxsize=None)
def _oracle(lag, n, h_signed, train_ar):
    """(sum LL, d/dh, L1 mass of d/dh, d/d mat, the per-entry bound of d/d mat) of the oracle."""
    codes, counts, mat, oh, f = _inputs(lag, n)
    if not len(codes):
        z = np.zeros((lag, W, W))
        return 0.0, 0.0, 0.0, z, z
    r = o.bear_net_step(counts, f, h_signed, train_ar=train_ar)
    mass, gm = co.dm_prior_mass_w(counts, f, h_signed, train_ar=train_ar, want_grad=True)
    G = _chain(oh, f, r["d_prior"])
    delta = CELL_RTOL * gm
    tol = GRAD_RTOL * np.abs(G).max() + np.einsum("njk,nl->jkl", oh, f * (delta + (f * delta).sum(-1, keepdims=True)))
    return r["ll"], (0.0 if train_ar else r["d_h_signed"]), mass[0], G, tol


def _primitive(lag, n, h_signed, train_ar):
    codes, counts, mat, _, _ = _inputs(lag, n)
    out, grad = kernels.dm_linear_wide(_dev_counts(counts), _dev(codes), _dev(mat), h_signed, train_ar=train_ar)
    return out.cpu().numpy(), grad.cpu().numpy()


# ------------------------------------------------------------------ 1. the primitive against the oracle
@pytest.mark.parametrize("lag,n", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("train_ar", [False, True])
@pytest.mark.parametrize("h_signed", H_SIGNED)
def test_primitive_matches_oracle(lag, n, train_ar, h_signed):
    ll, dh, dh_mass, G, tol = _oracle(lag, n, h_signed, train_ar)
    out, grad = _primitive(lag, n, h_signed, train_ar)
    assert grad.shape == (lag, W, W)
    if n == EMPTY:
        assert out.tolist() == [0.0, 0.0] and not grad.any()
        return
    print("sum LL rel", abs(out[0] / ll - 1) if ll else out[0], "d/dh", abs(out[1] - dh), "of", dh_mass,
          "d/d mat worst entry / bound", (np.abs(grad - G) / np.maximum(tol, 1e-300)).max())
    assert np.isclose(out[0], ll, rtol=1e-11, atol=0), (out[0], ll)
    if train_ar:
        assert out[1] == 0.0
    else:
        assert abs(out[1] - dh) <= 2e-13 * dh_mass, (out[1], dh, dh_mass)
    assert (np.abs(grad - G) <= tol).all(), (np.abs(grad - G) / np.maximum(tol, 1e-300)).max()


# ------------------------------------------------------------------ 2. ... and against the three launches it replaces
@pytest.mark.parametrize("lag,n", SHAPES, ids=_shape_id)
def test_fused_equals_the_three_launches(lag, n):
    """Not bit for bit: the three kernels cut the table into other tiles on other grids (forward 512 contexts on one block per CU,
    the DM step four blocks per CU, the backward product its own partial rows), so the fixed-order sums add in another order."""
    codes, counts, mat, _, _ = _inputs(lag, n)
    d_codes, d_counts, d_mat = _dev(codes), _dev_counts(counts), _dev(mat)
    for train_ar in (False, True):
        for h_signed in H_SIGNED:
            h_dev = torch.tensor([h_signed], dtype=torch.float64, device="cuda")
            prior = kernels.linear_forward_wide(d_codes, d_mat, lag)
            want, q = kernels.dm_prior_wide(d_counts, prior, h_dev, train_ar=train_ar, want_grad=True)
            want_g = kernels.linear_backward_wide(d_codes, lag, prior, q).cpu().numpy()
            want = want.cpu().numpy()
            out, grad = _primitive(lag, n, h_signed, train_ar)
            if n == EMPTY:
                assert out.tolist() == [0.0, 0.0] and not grad.any() and not want_g.any()
                continue
            tol = _oracle(lag, n, h_signed, train_ar)[4]
            assert np.isclose(out[0], want[0], rtol=1e-12, atol=0), (out[0], want[0])
            assert np.isclose(out[1], want[1], rtol=1e-12, atol=0), (out[1], want[1])
            assert (np.abs(grad - want_g) <= tol).all(), (np.abs(grad - want_g) / np.maximum(tol, 1e-300)).max()


def test_contexts_without_counts_add_exact_zeros():
    lag, n = 6, 700
    rng = np.random.default_rng(17)
    codes, mat = _codes(n, lag, rng), rng.normal(size=(lag, W, W)) * 0.4
    counts = _counts(n, rng)
    codes[codes == 7] = 8                      # letter 7 never occurs: its rows of d/d mat are exactly zero
    for train_ar in (False, True):
        out, grad = kernels.dm_linear_wide(_dev_counts(counts), _dev(codes), _dev(mat), 0.3, train_ar=train_ar)
        live = counts.any(1)
        out2, grad2 = kernels.dm_linear_wide(_dev_counts(counts[live]), _dev(codes[live]), _dev(mat), 0.3, train_ar=train_ar)
        assert np.all(grad.cpu().numpy()[:, 7, :] == 0.0)
        assert np.isclose(out[0].item(), out2[0].item(), rtol=1e-12) and np.isclose(out[1].item(), out2[1].item(), rtol=1e-12)
        top = float(grad2.abs().max())
        assert float((grad - grad2).abs().max()) <= GRAD_RTOL * top
        z, gz = kernels.dm_linear_wide(_dev_counts(np.zeros_like(counts)), _dev(codes), _dev(mat), 0.3, train_ar=train_ar)
        assert z.tolist() == [0.0, 0.0] and not gz.any()


# ------------------------------------------------------------------ 3. repeatability
_REPEAT = (
    "import hashlib\nimport numpy as np, torch\nfrom bear_amd import kernels\n"
    "def digest():\n"
    "    rng = np.random.default_rng(8)\n"
    "    lag, n = 12, 20011\n"
    "    codes = rng.integers(-1, 21, size=(n, lag)).astype(np.int8)\n"
    "    c = np.where(rng.random((n, 21)) < 0.15, rng.poisson(rng.uniform(0.5, 40.0, (n, 1)), (n, 21)), 0).astype(np.uint32)\n"
    "    c[rng.random(n) < 0.3] = 0\n"
    "    mat = torch.from_numpy(rng.normal(size=(lag, 21, 21)) * 0.4).cuda()\n"
    "    cd, kd = torch.from_numpy(c.view(np.int32)).cuda(), torch.from_numpy(codes).cuda()\n"
    "    h = hashlib.sha256()\n"
    "    for ar in (False, True):\n"
    "        a = [x.cpu().numpy().tobytes() for x in kernels.dm_linear_wide(cd, kd, mat, 0.2, train_ar=ar)]\n"
    "        b = [x.cpu().numpy().tobytes() for x in kernels.dm_linear_wide(cd, kd, mat, 0.2, train_ar=ar)]\n"
    "        assert a == b and any(a[1])\n"
    "        h.update(a[0] + a[1])\n"
    "    return h.hexdigest()\n")


def test_same_call_same_bytes_in_both_builds(tmp_path):
    scope = {}
    exec(compile(_REPEAT, "repeat", "exec"), scope)
    mine = scope["digest"]()
    script = tmp_path / "det_linear_step_wide.py"
    script.write_text("import sys\nsys.path.insert(0, sys.argv[1])\n"
                      "from bear_amd import _lib\nassert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH\n"
                      + _REPEAT + "print('DET_LINEAR_STEP_WIDE', digest())\n")
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "DET_LINEAR_STEP_WIDE" in p.stdout, p.stdout + p.stderr
    assert p.stdout.split("DET_LINEAR_STEP_WIDE")[1].split()[0] == mine


# ------------------------------------------------------------------ 4. the reduce and step forms
def _theta(lag, mat, h_signed):
    return torch.cat([torch.tensor([h_signed], dtype=torch.float64), torch.from_numpy(mat).reshape(-1)]).cuda()


@pytest.mark.parametrize("lag,n", [(3, 129), (5, 1365), (MAX_LAG, 257), (4, EMPTY)], ids=_shape_id)
@pytest.mark.parametrize("train_ar", [False, True])
def test_reduce_and_step(lag, n, train_ar, monkeypatch):
    codes, counts, mat, _, _ = _inputs(lag, n)
    d_codes, d_counts = _dev(codes), _dev_counts(counts)
    size = 1 + lag * W * W
    theta = _theta(lag, mat, 0.3)
    out, grad = _primitive(lag, n, 0.3, train_ar)
    packed = torch.full((size + 1,), 7.0, dtype=torch.float64, device="cuda")
    kernels.net_linear_train_reduce_wide(d_counts, d_codes, lag, theta, packed, train_ar=train_ar)
    assert packed.cpu().numpy().tobytes() == np.concatenate([out, grad.reshape(-1)]).tobytes()
    # the step form: reduce, then bear_train_apply_f64 -- three optimizer steps, the loss record included
    def run(step_form):
        th = _theta(lag, mat, 0.3)
        m, v, t = torch.zeros_like(th), torch.zeros_like(th), torch.zeros(1, dtype=torch.float64, device="cuda")
        pk, loss = torch.zeros(size + 1, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
        for _ in range(3):
            if step_form:
                kernels.net_linear_train_step_wide(d_counts, d_codes, lag, th, m, v, t, pk, 0.01, -2.5, loss, train_ar=train_ar)
            else:
                kernels.net_linear_train_reduce_wide(d_counts, d_codes, lag, th, pk, train_ar=train_ar)
                kernels.train_apply(th, pk, m, v, t, 0.01, -2.5, loss, train_ar=train_ar)
        return [x.cpu().numpy().tobytes() for x in (th, m, v, t, loss, pk)]
    want = run(False)
    assert run(True) == want
    monkeypatch.setenv("BEAR_AMD_TWO_LAUNCH_STEP", "1")
    assert run(True) == want
    th = np.frombuffer(want[0])
    assert np.frombuffer(want[3])[0] == 3.0 and np.frombuffer(want[4])[3] == 0.0
    if train_ar:
        assert th[0] == 0.3                    # AR mode: h_signed receives no update
    elif n != EMPTY:
        assert th[0] != 0.3
    if n != EMPTY:
        assert np.abs(th[1:] - mat.reshape(-1)).max() > 0 and np.frombuffer(want[4])[:3].all()


@pytest.mark.parametrize("train_ar", [False, True])
def test_halves_add_up(train_ar):
    """The multi-rank contract: packed of a table is the sum of the packed vectors of its pieces."""
    lag, n = 5, 1365
    codes, counts, mat, _, _ = _inputs(lag, n)
    theta, size = _theta(lag, mat, 0.3), 1 + lag * W * W
    parts = []
    for a, b in ((0, n), (0, n // 2), (n // 2, n)):
        packed = torch.zeros(size + 1, dtype=torch.float64, device="cuda")
        kernels.net_linear_train_reduce_wide(_dev_counts(counts[a:b]), _dev(codes[a:b]), lag, theta, packed, train_ar=train_ar)
        parts.append(packed.cpu().numpy())
    whole, two = parts[0], parts[1] + parts[2]
    _, _, dh_mass, _, tol = _oracle(lag, n, 0.3, train_ar)
    assert np.isclose(whole[0], two[0], rtol=1e-12, atol=0)
    assert abs(whole[1] - two[1]) <= 2e-13 * dh_mass + 1e-12 * abs(whole[1])
    assert (np.abs(whole[2:] - two[2:]) <= tol.reshape(-1)).all()


# ------------------------------------------------------------------ 5. the raw ABI's refusals
def test_raw_abi_refusals():
    L, p = _lib.lib(), kernels._ptr
    ws = kernels.default_workspace(torch.device("cuda", 0))
    n, lag = 64, 3
    counts = torch.ones((n + 1, W), dtype=torch.int32, device="cuda")
    codes = torch.zeros((n, MAX_LAG + 1), dtype=torch.int8, device="cuda")
    mat = torch.zeros((MAX_LAG + 1, W, W), dtype=torch.float64, device="cuda")
    theta = torch.zeros(1 + (MAX_LAG + 1) * W * W, dtype=torch.float64, device="cuda")
    packed = torch.full((2 + (MAX_LAG + 1) * W * W,), 7.0, dtype=torch.float64, device="cuda")
    out, grad = packed[:2], torch.full_like(mat, 7.0)

    def prim(counts_p=p(counts), codes_p=p(codes), lag=lag, width=W, mat_p=p(mat), out_p=p(out), grad_p=p(grad)):
        return L.bear_dm_linear_wide_f64(ws.handle, counts_p, codes_p, n, lag, width, mat_p, 0.0, EPS, 0, out_p, grad_p, None)

    def reduce(counts_p=p(counts), codes_p=p(codes), lag=lag, width=W, theta_p=p(theta), packed_p=p(packed)):
        return L.bear_net_linear_train_reduce_wide_f64(ws.handle, counts_p, codes_p, n, lag, width, theta_p, EPS, 0, packed_p, None)

    def step(counts_p=p(counts), codes_p=p(codes), lag=lag, width=W, theta_p=p(theta), m_p=p(theta), packed_p=p(packed)):
        return L.bear_net_linear_train_step_wide_f64(ws.handle, counts_p, codes_p, n, lag, width, theta_p, m_p, p(theta), p(theta), EPS, 0,
                                                     0.01, 1.0, packed_p, None, 0, None)
    misaligned = kernels.ctypes.c_void_p(counts.data_ptr() + 4)
    for fn in (prim, reduce, step):
        for kw in ({"width": 5}, {"width": 7}, {"lag": 0}, {"lag": MAX_LAG + 1}, {"counts_p": None}, {"codes_p": None},
                   {"counts_p": misaligned}):
            assert fn(**kw) == -1, (fn.__name__, kw)
    assert prim(mat_p=None) == -1 and prim(out_p=None) == -1 and prim(grad_p=None) == -1
    assert reduce(theta_p=None) == -1 and reduce(packed_p=None) == -1
    assert step(theta_p=None) == -1 and step(m_p=None) == -1 and step(packed_p=None) == -1
    torch.cuda.synchronize()
    assert (packed == 7.0).all() and (grad == 7.0).all() and not theta.any()      # nothing was launched
    with pytest.raises(ValueError):
        kernels.dm_linear_wide(counts[:n], codes[:, :lag].contiguous(), torch.zeros((lag, 5, 5), dtype=torch.float64, device="cuda"), 0.0)


# ------------------------------------------------------------------ 6. bear_net.train on a protein table
N_ROWS, BATCH, LAG, EPOCHS = 400, 150, 4, 6


@pytest.fixture
def prot(tmp_path):
    kmers, counts = make_prot_table(seed=0, n=N_ROWS, num_ds=3)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    return dataloader.dataloader(str(path), "prot", BATCH, 3), kmers, counts


def _spy(monkeypatch, calls, *names):
    for name in names:
        def wrapper(*a, _real=getattr(kernels, name), _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a, **kw)
        monkeypatch.setattr(kernels, name, wrapper)


def _train_run(data, n, train_ar=False, optimizer="Adam", lr=0.01, epochs=EPOCHS, **kw):
    torch.manual_seed(1)
    losses = []
    params, _, _ = bear_net.train(data.repeat(epochs), n, epochs, 0, "prot", LAG, ar_funcs.make_ar_func_linear, {}, lr, optimizer, train_ar,
                                  loss_save=losses, **kw)
    return np.array(losses), [p.detach().cpu().numpy() for p in params]


def _same(a, b):
    assert np.allclose(a[0], b[0], rtol=1e-9, atol=0), np.abs(a[0] / b[0] - 1).max()
    for x, y in zip(a[1], b[1]):
        assert np.allclose(x, y, rtol=1e-7, atol=1e-9)


def test_train_takes_the_fused_step(prot, monkeypatch):
    """The test that fails without the feature: bear_net.train with make_ar_func_linear on a protein table runs
    bear_net_linear_train_step_wide_f64 from a device-resident theta, not the three row kernels under autograd."""
    data, kmers, _ = prot
    calls = {}
    _spy(monkeypatch, calls, "net_linear_train_step_wide", "net_linear_train_reduce_wide", "linear_forward_wide", "dm_prior_wide")
    fused = _train_run(data, len(kmers))
    assert calls.get("net_linear_train_step_wide", 0) > 0 and "linear_forward_wide" not in calls and "dm_prior_wide" not in calls
    assert _train.LAST_RUN["graph"] and _train.LAST_RUN["one_launch_steps"]
    assert len(fused[0]) == 3 * EPOCHS
    calls.clear()
    monkeypatch.setenv("BEAR_AMD_UNFUSED_LINEAR_WIDE", "1")
    unfused = _train_run(data, len(kmers))
    assert calls.get("linear_forward_wide", 0) > 0 and "net_linear_train_step_wide" not in calls
    _same(fused, unfused)


@pytest.mark.parametrize("train_ar", [False, True])
def test_train_matches_numpy_loop(prot, train_ar):
    data, kmers, counts = prot
    n = len(kmers)
    torch.manual_seed(1)
    _, (mat0,) = ar_funcs.make_ar_func_linear(LAG, 20)
    got = _train_run(data, n, train_ar=train_ar, params_restart=[np.array(0.1), mat0.detach().numpy().copy()])
    oh = _onehot(np.asarray(data.codes()))
    h, mat = np.array(0.1), mat0.detach().numpy().copy()
    ms, vs = [np.zeros_like(h), np.zeros_like(mat)], [np.zeros_like(h), np.zeros_like(mat)]
    want_loss, t = [], 0
    for _ in range(EPOCHS):
        for a in range(0, n, BATCH):
            b = min(a + BATCH, n)
            f = o.ar_func_linear(oh[a:b], mat)
            r = o.bear_net_step(counts[0, a:b], f, float(h), train_ar=train_ar)
            scale = -(n / (b - a))
            want_loss.append(-scale * r["ll"])
            t += 1
            g_mat = scale * _chain(oh[a:b], f, r["d_prior"])
            if not train_ar:
                keras_adam_np(h, np.array(scale * r["d_h_signed"]), ms[0], vs[0], t)
            keras_adam_np(mat, g_mat, ms[1], vs[1], t)
    _same(got, (np.array(want_loss), [h, mat]))


def test_graph_replay_equals_eager_bytes(prot, monkeypatch):
    data, kmers, _ = prot
    graph = _train_run(data, len(kmers))
    assert _train.LAST_RUN["graph"]
    monkeypatch.setenv("BEAR_AMD_NO_GRAPH", "1")
    eager = _train_run(data, len(kmers))
    assert not _train.LAST_RUN["graph"]
    assert graph[0].tobytes() == eager[0].tobytes()
    for a, b in zip(graph[1], eager[1]):
        assert a.tobytes() == b.tobytes()
    monkeypatch.delenv("BEAR_AMD_NO_GRAPH")
    monkeypatch.setenv("BEAR_AMD_GRAPH_MAX_ROWS", "100")        # a cap that is set is honoured: batches of 150 rows run eagerly
    capped = _train_run(data, len(kmers))
    assert not _train.LAST_RUN["graph"] and capped[0].tobytes() == graph[0].tobytes()


@pytest.mark.parametrize("variant", ["acc_steps", "params_restart", "sgd"])
def test_train_variants_match_the_unfused_path(prot, variant, monkeypatch):
    data, kmers, _ = prot
    kw = {}
    if variant == "acc_steps":
        kw["acc_steps"] = 2
    elif variant == "params_restart":
        torch.manual_seed(5)
        _, (m0,) = ar_funcs.make_ar_func_linear(LAG, 20)
        kw["params_restart"] = [np.array(0.1), m0.detach().numpy()]
    else:
        kw.update(optimizer="SGD", lr=1e-7)       # (a step small enough for the table's largest counts)
    calls = {}
    _spy(monkeypatch, calls, "net_linear_train_step_wide", "net_linear_train_reduce_wide", "linear_forward_wide")
    fused = _train_run(data, len(kmers), **kw)
    assert "linear_forward_wide" not in calls and (calls.get("net_linear_train_step_wide", 0) + calls.get("net_linear_train_reduce_wide", 0)) > 0
    monkeypatch.setenv("BEAR_AMD_UNFUSED_LINEAR_WIDE", "1")
    unfused = _train_run(data, len(kmers), **kw)
    assert len(fused[0]) == len(unfused[0]) and np.allclose(fused[0], unfused[0], rtol=1e-9, atol=0)


def test_device_resident_table_trains_on_the_fused_step(tmp_path, monkeypatch):
    from test_prot_summarize_gpu import _two_fastas
    lst = _two_fastas(tmp_path, np.random.default_rng(5), n=100)
    lag = 3
    dev = summarize.count_tables(lst, lag, alphabet="prot", on_device=True)[lag - 1]
    host = summarize.count_tables(lst, lag, alphabet="prot")[lag - 1]
    calls = {}
    _spy(monkeypatch, calls, "net_linear_train_step_wide", "linear_forward_wide")
    runs = []
    for data in (dev, host):
        torch.manual_seed(0)
        ls = []
        bear_net.train(data.repeat(4), data.num_rows, 4, 0, "prot", lag, ar_funcs.make_ar_func_linear, {}, 0.01, "Adam", False, loss_save=ls)
        runs.append(np.array(ls))
    assert calls.get("net_linear_train_step_wide", 0) > 0 and "linear_forward_wide" not in calls
    assert len(runs[0]) == 4 and np.all(np.isfinite(runs[0])) and runs[0].tobytes() == runs[1].tobytes()


# ------------------------------------------------------------------ 7. two ranks
def test_two_ranks_match_one(prot, tmp_path):
    data, kmers, _ = prot
    torch.manual_seed(3)
    _, (m0,) = ar_funcs.make_ar_func_linear(LAG, 20)
    restart = [np.array(0.1), m0.detach().numpy()]
    np.savez(tmp_path / "restart.npz", linear=np.array(restart, dtype=object))
    out_file = tmp_path / "out.json"
    _launch([os.path.join(ROOT, "tests", "prot_linear_step_worker.py")],
            {"BEAR_RESTART": str(tmp_path / "restart.npz"), "BEAR_OUT": str(out_file), "BEAR_TABLE": str(tmp_path / "prot.tsv")}, tmp_path)
    got = json.load(open(out_file))
    for train_ar in (False, True):
        want = _train_run(data, len(kmers), train_ar=train_ar, params_restart=restart)
        g = got["ar" if train_ar else "bear"]
        assert g["step_fns"] == "wide"
        assert np.allclose(g["loss"], want[0], rtol=1e-10, atol=0)
        for a, b in zip(g["params"], want[1]):
            assert np.allclose(np.asarray(a), b, rtol=1e-7, atol=1e-10)
