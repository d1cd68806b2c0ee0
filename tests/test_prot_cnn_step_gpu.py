"""GPU tests of bear_net's step with the convolutional AR function at the protein alphabet's width as two launches
(bear_dm_cnn_wide_f64, bear_net_cnn_train_{reduce,step}_wide_f64; kernels_cnn_wide.h): the primitive against the oracle (ar_func_cnn
on a one-hot, bear_net_step, torch fp64 autograd of the one-hot formulation fed the oracle's gradient rows) and against the three
launches it replaces -- both held to the same bounds on the same inputs --, contexts without counts, equal bytes from call to call
and in the deterministic build, the reduce and step forms, the raw ABI's refusals, and bear_net.train on a protein table: alone,
against the unfused path, against the oracle loop, and on two ranks.  Tolerances: those of test_prot_linear_step_gpu.py for the two
sums, GRAD_RTOL of test_prot_cnn_rows_gpu.py (1e-10 of a parameter tensor's largest entry) for the gradients."""
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
from bear_amd import _lib, _train, ar_funcs, bear_net, dataloader, kernels
from conftest import ROOT
from test_dist_gpu import _launch
from test_prot_cpu import make_prot_table, write_prot_tsv
from test_prot_gpu import keras_adam_np
from test_prot_linear_rows_gpu import _codes, _onehot
from test_prot_linear_step_gpu import _counts, _dev, _dev_counts, _same, _spy
from test_prot_cnn_rows_gpu import GRAD_RTOL, _autograd_reference, _flat, _make, _np

pytestmark = pytest.mark.gpu

W = 21
EPS = 1e-7
MAX_LAG = kernels.CNN_WIDE_MAX_LAG
T = kernels.CNN_STEP_WIDE_TILE
BWD_TILE = kernels.CNN_STEP_WIDE_BACKWARD_TILE
GRID_CAP = "one tile more than the larger of the two capped grids holds, and then some: a block of either kernel takes more than one"
EMPTY = 0
SHAPES = [(1, 1, 1), (1, 1, 70), (4, 1, 64), (5, 3, 65), (6, 4, 63), (6, 4, T - 1), (6, 4, T), (6, 4, T + 1), (8, 8, 130), (12, 8, 1365),
          (16, 8, 257), (16, 16, 65), (16, 1, 129), (3, 2, GRID_CAP), (4, 2, EMPTY)]
H_SIGNED = [-3.0, 0.0, 2.0]


def _shape_id(v):
    return "cap" if v is GRID_CAP else str(v)


def _n(n):
    if n is GRID_CAP:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        head = cus * kernels.CNN_STEP_WIDE_BLOCKS_PER_CU * T + T
        back = cus * kernels.CNN_STEP_WIDE_BACKWARD_BLOCKS_PER_CU * BWD_TILE + BWD_TILE
        return max(head, back) + 5 * BWD_TILE + 77
    return n


@functools.lru_cache(maxsize=None)
def _inputs(lag, fw, n):
    """One seeded problem per shape, shared by the tests (read-only): codes, counts, the one-hot, the oracle's rows; the AR function
    (every parameter moved off its initial value) and its parameters on the device."""
    n = _n(n)
    rng = np.random.default_rng(lag * 1000 + fw * 100 + n)
    codes = _codes(n, lag, rng)
    counts = _counts(n, rng)
    ar_func, params = _make(lag, fw, 3)
    oh = _onehot(codes)
    f = o.ar_func_cnn(oh, _np(params)) if n else np.zeros((0, W))
    for a in (codes, counts, oh, f):
        a.setflags(write=False)
    return codes, counts, oh, f, ar_func, params


@functools.lru_cache(maxsize=None)
def _oracle(lag, fw, n, h_signed, train_ar):
    """(sum LL, d/dh, L1 mass of d/dh, d/d flat parameters) of the oracle: bear_net_step on the oracle's rows, its gradient rows carried
    to the parameters by torch fp64 autograd of the one-hot formulation."""
    codes, counts, oh, f, ar_func, params = _inputs(lag, fw, n)
    if not len(codes):
        return 0.0, 0.0, 0.0, torch.zeros_like(_flat(params))
    r = o.bear_net_step(counts, f, h_signed, train_ar=train_ar)
    mass, _ = co.dm_prior_mass_w(counts, f, h_signed, train_ar=train_ar)
    _, want_g = _autograd_reference(ar_func, params, _dev(oh), _dev(r["d_prior"]))
    return r["ll"], (0.0 if train_ar else r["d_h_signed"]), mass[0], want_g


def _grad_excess(got, want, params):
    """The largest |got - want| of a parameter tensor over GRAD_RTOL times that tensor's largest entry of `want`: <= 1 passes."""
    worst, k = 0.0, 0
    for p in params:
        m = p.numel()
        err = (got[k:k + m] - want[k:k + m]).abs().max().item()
        top = max(want[k:k + m].abs().max().item(), 1e-300)
        worst = max(worst, err / (GRAD_RTOL * top))
        k += m
    return worst


def _primitive(lag, fw, n, h_signed, train_ar, bufs=None):
    codes, counts, _, _, _, params = _inputs(lag, fw, n)
    return kernels.dm_cnn_wide(_dev_counts(counts), _dev(codes), _flat(params), lag, fw, h_signed, train_ar=train_ar, bufs=bufs)


def _three_launches(lag, fw, n, h_signed, train_ar):
    codes, counts, _, _, _, params = _inputs(lag, fw, n)
    d_codes, flat = _dev(codes), _flat(params)
    h_dev = torch.tensor([h_signed], dtype=torch.float64, device="cuda")
    prior, t1 = kernels.cnn_forward_wide(d_codes, flat, lag, fw)
    out, q = kernels.dm_prior_wide(_dev_counts(counts), prior, h_dev, train_ar=train_ar, want_grad=True)
    return out, kernels.cnn_backward_wide(d_codes, flat, lag, fw, t1, prior, q)


def _assert_against_oracle(what, out, grad, want, params, train_ar):
    ll, dh, dh_mass, want_g = want
    out = out.cpu().numpy()
    excess = _grad_excess(grad, want_g, params)
    print(what, "sum LL rel", abs(out[0] / ll - 1) if ll else out[0], "d/dh", abs(out[1] - dh), "of", dh_mass, "gradient / bound", excess)
    assert np.isclose(out[0], ll, rtol=1e-11, atol=0), (what, out[0], ll)
    if train_ar:
        assert out[1] == 0.0, what
    else:
        assert abs(out[1] - dh) <= 2e-13 * dh_mass, (what, out[1], dh, dh_mass)
    assert excess <= 1.0, (what, excess)


# ------------------------------------------------------------------ 1. the primitive against the oracle
@pytest.mark.parametrize("lag,fw,n", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("train_ar", [False, True])
def test_primitive_matches_oracle(lag, fw, n, train_ar):
    params = _inputs(lag, fw, n)[5]
    for h_signed in H_SIGNED:
        out, grad = _primitive(lag, fw, n, h_signed, train_ar)
        assert grad.shape == (kernels.cnn_param_count_wide(lag, fw),)
        if n == EMPTY:
            assert out.tolist() == [0.0, 0.0] and not grad.any()
            continue
        want = _oracle(lag, fw, n, h_signed, train_ar)
        _assert_against_oracle("fused", out, grad, want, params, train_ar)
        # the three launches it replaces, on the same input, to the same bounds
        _assert_against_oracle("three launches", *_three_launches(lag, fw, n, h_signed, train_ar), want, params, train_ar)


# ------------------------------------------------------------------ 2. ... and against the three launches it replaces
@pytest.mark.parametrize("lag,fw,n", SHAPES, ids=_shape_id)
def test_fused_equals_the_three_launches(lag, fw, n):
    """Not bit for bit: the head kernel cuts the table into tiles of 256 on one block per CU, dm_wide_kernel into tiles of 128 on
    four, so the fixed-order sums add in another order (and dz is formed from a row that never left the CU)."""
    params = _inputs(lag, fw, n)[5]
    for train_ar in (False, True):
        for h_signed in H_SIGNED:
            out, grad = _primitive(lag, fw, n, h_signed, train_ar)
            want, want_g = _three_launches(lag, fw, n, h_signed, train_ar)
            if n == EMPTY:
                assert out.tolist() == [0.0, 0.0] and not grad.any() and not want_g.any()
                continue
            out, want = out.cpu().numpy(), want.cpu().numpy()
            assert np.isclose(out[0], want[0], rtol=1e-12, atol=0), (out[0], want[0])
            assert np.isclose(out[1], want[1], rtol=1e-12, atol=0), (out[1], want[1])
            assert _grad_excess(grad, want_g, params) <= 1.0


# ------------------------------------------------------------------ 3. contexts without counts
def test_contexts_without_counts_add_exact_zeros():
    lag, fw, n = 6, 3, 700
    rng = np.random.default_rng(17)
    codes, counts = _codes(n, lag, rng), _counts(n, rng)
    codes[codes == 7] = 8                      # letter 7 never occurs: its filter-gradient rows are exactly zero
    _, params = _make(lag, fw, 5)
    flat = _flat(params)
    live = counts.any(1)
    assert 0 < live.sum() < n
    for train_ar in (False, True):
        bufs = tuple(torch.full_like(b, 7.0) for b in kernels.cnn_step_buffers_wide(n, "cuda"))
        out, grad = kernels.dm_cnn_wide(_dev_counts(counts), _dev(codes), flat, lag, fw, 0.3, train_ar=train_ar, bufs=bufs)
        dz = bufs[0].cpu().numpy()
        assert np.all(dz[~live] == 0.0) and np.abs(dz[live]).max() > 0 and np.all(np.isfinite(bufs[1].cpu().numpy()))
        out2, grad2 = kernels.dm_cnn_wide(_dev_counts(counts[live]), _dev(codes[live]), flat, lag, fw, 0.3, train_ar=train_ar)
        assert np.isclose(out[0].item(), out2[0].item(), rtol=1e-12) and np.isclose(out[1].item(), out2[1].item(), rtol=1e-12)
        assert _grad_excess(grad, grad2, params) <= 1.0
        gf = grad[:fw * W * 30].reshape(fw, W, 30).cpu().numpy()
        assert np.abs(gf).max() > 0 and np.all(gf[:, 7, :] == 0.0)
        z, gz = kernels.dm_cnn_wide(_dev_counts(np.zeros_like(counts)), _dev(codes), flat, lag, fw, 0.3, train_ar=train_ar, bufs=bufs)
        assert z.tolist() == [0.0, 0.0] and not gz.any() and not bufs[0].any()


# ------------------------------------------------------------------ 4. repeatability
_REPEAT = (
    "import hashlib\nimport numpy as np, torch\nfrom bear_amd import kernels\n"
    "def digest():\n"
    "    rng = np.random.default_rng(8)\n"
    "    lag, fw, n = 12, 8, 20011\n"
    "    codes = rng.integers(-1, 21, size=(n, lag)).astype(np.int8)\n"
    "    c = np.where(rng.random((n, 21)) < 0.15, rng.poisson(rng.uniform(0.5, 40.0, (n, 1)), (n, 21)), 0).astype(np.uint32)\n"
    "    c[rng.random(n) < 0.3] = 0\n"
    "    flat = torch.from_numpy(rng.normal(size=kernels.cnn_param_count_wide(lag, fw)) * 0.3).cuda()\n"
    "    cd, kd = torch.from_numpy(c.view(np.int32)).cuda(), torch.from_numpy(codes).cuda()\n"
    "    h = hashlib.sha256()\n"
    "    for ar in (False, True):\n"
    "        a = [x.cpu().numpy().tobytes() for x in kernels.dm_cnn_wide(cd, kd, flat, lag, fw, 0.2, train_ar=ar)]\n"
    "        b = [x.cpu().numpy().tobytes() for x in kernels.dm_cnn_wide(cd, kd, flat, lag, fw, 0.2, train_ar=ar)]\n"
    "        assert a == b and any(a[1])\n"
    "        h.update(a[0] + a[1])\n"
    "    return h.hexdigest()\n")


def test_same_call_same_bytes_in_both_builds(tmp_path):
    scope = {}
    exec(compile(_REPEAT, "repeat", "exec"), scope)
    mine = scope["digest"]()
    script = tmp_path / "det_cnn_step_wide.py"
    script.write_text("import sys\nsys.path.insert(0, sys.argv[1])\n"
                      "from bear_amd import _lib\nassert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH\n"
                      + _REPEAT + "print('DET_CNN_STEP_WIDE', digest())\n")
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "DET_CNN_STEP_WIDE" in p.stdout, p.stdout + p.stderr
    assert p.stdout.split("DET_CNN_STEP_WIDE")[1].split()[0] == mine


# ------------------------------------------------------------------ 5. the reduce and step forms
def _theta(params, h_signed):
    return torch.cat([torch.tensor([h_signed], dtype=torch.float64, device="cuda"), _flat(params)]).contiguous()


@pytest.mark.parametrize("lag,fw,n", [(3, 2, 129), (5, 3, 1365), (MAX_LAG, 8, 257), (4, 2, EMPTY)], ids=_shape_id)
@pytest.mark.parametrize("train_ar", [False, True])
def test_reduce_and_step(lag, fw, n, train_ar, monkeypatch):
    codes, counts, _, _, _, params = _inputs(lag, fw, n)
    d_codes, d_counts = _dev(codes), _dev_counts(counts)
    bufs = kernels.cnn_step_buffers_wide(len(codes), "cuda")
    theta = _theta(params, 0.3)
    size = theta.numel()
    out, grad = _primitive(lag, fw, n, 0.3, train_ar)
    packed = torch.full((size + 1,), 7.0, dtype=torch.float64, device="cuda")
    kernels.net_cnn_train_reduce_wide(d_counts, d_codes, lag, fw, theta, bufs, packed, train_ar=train_ar)
    assert packed.cpu().numpy().tobytes() == torch.cat([out, grad]).cpu().numpy().tobytes()

    def run(step_form):
        th = _theta(params, 0.3)
        m, v, t = torch.zeros_like(th), torch.zeros_like(th), torch.zeros(1, dtype=torch.float64, device="cuda")
        pk, loss = torch.zeros(size + 1, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
        for _ in range(3):
            if step_form:
                kernels.net_cnn_train_step_wide(d_counts, d_codes, lag, fw, th, m, v, t, bufs, pk, 0.01, -2.5, loss, train_ar=train_ar)
            else:
                kernels.net_cnn_train_reduce_wide(d_counts, d_codes, lag, fw, th, bufs, pk, train_ar=train_ar)
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
        assert np.abs(th[1:] - theta[1:].cpu().numpy()).max() > 0 and np.frombuffer(want[4])[:3].all()


@pytest.mark.parametrize("train_ar", [False, True])
def test_halves_add_up(train_ar):
    """The multi-rank contract: packed of a table is the sum of the packed vectors of its pieces."""
    lag, fw, n = 5, 3, 1365
    codes, counts, _, _, _, params = _inputs(lag, fw, n)
    theta = _theta(params, 0.3)
    bufs = kernels.cnn_step_buffers_wide(n, "cuda")
    parts = []
    for a, b in ((0, n), (0, n // 2), (n // 2, n)):
        packed = torch.zeros(theta.numel() + 1, dtype=torch.float64, device="cuda")
        kernels.net_cnn_train_reduce_wide(_dev_counts(counts[a:b]), _dev(codes[a:b]), lag, fw, theta, bufs, packed, train_ar=train_ar)
        parts.append(packed.clone())
    whole, two = parts[0], parts[1] + parts[2]
    dh_mass = _oracle(lag, fw, n, 0.3, train_ar)[2]
    assert np.isclose(whole[0].item(), two[0].item(), rtol=1e-12, atol=0)
    assert abs(whole[1].item() - two[1].item()) <= 2e-13 * dh_mass + 1e-12 * abs(whole[1].item())
    assert _grad_excess(two[2:], whole[2:], params) <= 1.0


# ------------------------------------------------------------------ 6. the raw ABI's refusals
def test_raw_abi_refusals():
    L, p = _lib.lib(), kernels._ptr
    ws = kernels.default_workspace(torch.device("cuda", 0))
    n, lag, fw = 64, 5, 3
    counts = torch.ones((n + 1, W), dtype=torch.int32, device="cuda")
    codes = torch.zeros((n, MAX_LAG + 1), dtype=torch.int8, device="cuda")
    size = 1 + kernels.cnn_param_count_wide(MAX_LAG, MAX_LAG) + 630
    theta = torch.zeros(size, dtype=torch.float64, device="cuda")
    packed = torch.full((size + 1,), 7.0, dtype=torch.float64, device="cuda")
    dz, t1 = torch.full((n + 1, W), 7.0, dtype=torch.float64, device="cuda"), torch.full((n + 1, 16), 7.0, dtype=torch.float64, device="cuda")
    out, grad = packed[:2], torch.full((size,), 7.0, dtype=torch.float64, device="cuda")
    base = dict(counts_p=p(counts), codes_p=p(codes), lag=lag, fw=fw, nf=30, l1=16, width=W, dz_p=p(dz), t1_p=p(t1))

    def prim(par_p=p(theta), out_p=p(out), grad_p=p(grad), **kw):
        a = dict(base, **kw)
        return L.bear_dm_cnn_wide_f64(ws.handle, a["counts_p"], a["codes_p"], n, a["lag"], a["fw"], a["nf"], a["l1"], a["width"], par_p, 0.0,
                                      EPS, 0, a["dz_p"], a["t1_p"], out_p, grad_p, None)

    def reduce(theta_p=p(theta), packed_p=p(packed), **kw):
        a = dict(base, **kw)
        return L.bear_net_cnn_train_reduce_wide_f64(ws.handle, a["counts_p"], a["codes_p"], n, a["lag"], a["fw"], a["nf"], a["l1"], a["width"],
                                                    theta_p, a["dz_p"], a["t1_p"], EPS, 0, packed_p, None)

    def step(theta_p=p(theta), m_p=p(theta), packed_p=p(packed), **kw):
        a = dict(base, **kw)
        return L.bear_net_cnn_train_step_wide_f64(ws.handle, a["counts_p"], a["codes_p"], n, a["lag"], a["fw"], a["nf"], a["l1"], a["width"],
                                                  theta_p, m_p, p(theta), p(theta), a["dz_p"], a["t1_p"], EPS, 0, 0.01, 1.0, packed_p, None, 0,
                                                  None)
    off = lambda t, k: kernels.ctypes.c_void_p(t.data_ptr() + k)
    for fn in (prim, reduce, step):
        for kw in ({"width": 5}, {"width": 7}, {"nf": 20}, {"l1": 8}, {"fw": 0}, {"fw": lag + 1}, {"lag": 0, "fw": 0},
                   {"lag": MAX_LAG + 1}, {"lag": MAX_LAG + 1, "fw": MAX_LAG + 1},
                   {"counts_p": None}, {"codes_p": None}, {"dz_p": None}, {"t1_p": None},
                   {"counts_p": off(counts, 4)}, {"codes_p": off(codes, 1)}, {"dz_p": off(dz, 8)}, {"t1_p": off(t1, 8)}):
            assert fn(**kw) == -1, (fn.__name__, kw)
    assert prim(par_p=None) == -1 and prim(out_p=None) == -1 and prim(grad_p=None) == -1 and prim(grad_p=off(grad, 4)) == -1
    assert reduce(theta_p=None) == -1 and reduce(packed_p=None) == -1 and reduce(theta_p=off(theta, 4)) == -1
    assert step(theta_p=None) == -1 and step(m_p=None) == -1 and step(packed_p=None) == -1
    torch.cuda.synchronize()
    assert (packed == 7.0).all() and (grad == 7.0).all() and (dz == 7.0).all() and (t1 == 7.0).all() and not theta.any()   # nothing was launched
    with pytest.raises(ValueError):
        kernels.dm_cnn_wide(counts[:n], codes[:, :lag].contiguous(), theta[:10], lag, fw, 0.0)          # a wrong parameter count
    with pytest.raises(ValueError):
        kernels.dm_cnn_wide(counts[:n], codes[:, :lag].contiguous(), theta[:kernels.cnn_param_count_wide(lag, fw)], lag, fw, 0.0,
                            bufs=(dz[:n - 1], t1))                                                     # buffers of fewer rows


# ------------------------------------------------------------------ 7. bear_net.train on a protein table
N_ROWS, BATCH, LAG, FW, EPOCHS = 400, 150, 4, 3, 6
ROWS_PATH = ("cnn_forward_wide", "dm_prior_wide")
STEP_PATH = ("net_cnn_train_step_wide", "net_cnn_train_reduce_wide")


@pytest.fixture
def prot(tmp_path):
    kmers, counts = make_prot_table(seed=0, n=N_ROWS, num_ds=3)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    return dataloader.dataloader(str(path), "prot", BATCH, 3), kmers, counts


def _train_run(data, n, train_ar=False, optimizer="Adam", lr=0.01, epochs=EPOCHS, **kw):
    torch.manual_seed(1)
    losses = []
    params, _, _ = bear_net.train(data.repeat(epochs), n, epochs, 0, "prot", LAG, ar_funcs.make_ar_func_cnn, {"filter_width": FW}, lr, optimizer,
                                  train_ar, loss_save=losses, **kw)
    return np.array(losses), [p.detach().cpu().numpy() for p in params]


def test_train_takes_the_fused_step(prot, monkeypatch):
    """The test that fails without the feature: bear_net.train with make_ar_func_cnn on a protein table runs
    bear_net_cnn_train_step_wide_f64 from a device-resident theta, not the row kernels under autograd."""
    data, kmers, _ = prot
    calls = {}
    _spy(monkeypatch, calls, *STEP_PATH, *ROWS_PATH)
    fused = _train_run(data, len(kmers))
    assert calls.get("net_cnn_train_step_wide", 0) > 0 and not any(k in calls for k in ROWS_PATH)
    assert _train.LAST_RUN["graph"] and _train.LAST_RUN["one_launch_steps"]
    assert len(fused[0]) == 3 * EPOCHS
    calls.clear()
    monkeypatch.setenv("BEAR_AMD_UNFUSED_CNN_WIDE", "1")
    unfused = _train_run(data, len(kmers))
    assert calls.get("cnn_forward_wide", 0) > 0 and calls.get("dm_prior_wide", 0) > 0 and not any(k in calls for k in STEP_PATH)
    _same(fused, unfused)


@pytest.mark.parametrize("train_ar", [False, True])
def test_train_matches_oracle_loop(prot, train_ar):
    """test_bear_net_train_prot_matches_oracle_loop for the convolutional function: the torch one-hot formulation on the host, the
    oracle's step, NumPy tf.keras Adam."""
    data, kmers, counts = prot
    n = len(kmers)
    torch.manual_seed(3)
    _, init = ar_funcs.make_ar_func_cnn(LAG, 20, filter_width=FW)
    init_np = [x.detach().numpy().copy() for x in init]
    got = _train_run(data, n, train_ar=train_ar, params_restart=[np.array(0.1)] + init_np)
    assert _train.LAST_RUN["graph"]
    f_cpu, p_cpu = ar_funcs.make_ar_func_cnn(LAG, 20, filter_width=FW)
    with torch.no_grad():
        for a, b in zip(p_cpu, init_np):
            a.copy_(torch.as_tensor(b))
    h = np.array(0.1)
    ms = [np.zeros_like(h)] + [np.zeros(x.shape) for x in p_cpu]
    vs = [np.zeros_like(h)] + [np.zeros(x.shape) for x in p_cpu]
    codes, c0 = torch.as_tensor(data.codes()), counts[0]
    want_loss, t = [], 0
    for _ in range(EPOCHS):
        for a in range(0, n, BATCH):
            b = min(a + BATCH, n)
            for q in p_cpu:
                q.grad = None
            prior = f_cpu(codes[a:b])
            r = o.bear_net_step(c0[a:b], prior.detach().numpy(), float(h), train_ar=train_ar)
            scale = -(n / (b - a))
            prior.backward(torch.as_tensor(scale * r["d_prior"]))
            want_loss.append(-scale * r["ll"])
            t += 1
            if not train_ar:
                keras_adam_np(h, np.array(scale * r["d_h_signed"]), ms[0], vs[0], t)
            for i, q in enumerate(p_cpu):
                keras_adam_np(q.detach().numpy(), q.grad.numpy(), ms[i + 1], vs[i + 1], t)
    assert len(got[0]) == len(want_loss) == 3 * EPOCHS
    assert np.allclose(got[0], want_loss, rtol=1e-9, atol=0)
    assert np.isclose(got[1][0].item(), float(h), rtol=1e-7, atol=1e-9)
    for x, y in zip(got[1][1:], p_cpu):
        assert np.allclose(x, y.detach().numpy(), rtol=1e-6, atol=1e-8)


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
        _, init = ar_funcs.make_ar_func_cnn(LAG, 20, filter_width=FW)
        kw["params_restart"] = [np.array(0.1)] + [x.detach().numpy() for x in init]
    else:
        kw.update(optimizer="SGD", lr=1e-7)       # (a step small enough for the table's largest counts)
    calls = {}
    _spy(monkeypatch, calls, *STEP_PATH, *ROWS_PATH)
    fused = _train_run(data, len(kmers), **kw)
    assert not any(k in calls for k in ROWS_PATH) and sum(calls.get(k, 0) for k in STEP_PATH) > 0
    monkeypatch.setenv("BEAR_AMD_UNFUSED_CNN_WIDE", "1")
    unfused = _train_run(data, len(kmers), **kw)
    assert len(fused[0]) == len(unfused[0]) and np.allclose(fused[0], unfused[0], rtol=1e-9, atol=0)


def test_streamed_epoch_gives_the_resident_losses(prot, monkeypatch):
    data, kmers, _ = prot
    resident = _train_run(data, len(kmers))
    assert not _train.LAST_RUN["streaming"]
    calls = {}
    _spy(monkeypatch, calls, *STEP_PATH, *ROWS_PATH)
    monkeypatch.setenv("BEAR_AMD_STREAM", "1")
    streamed = _train_run(data, len(kmers))
    assert _train.LAST_RUN["streaming"] and not _train.LAST_RUN["graph"]
    assert calls.get("net_cnn_train_reduce_wide", 0) > 0 and not any(k in calls for k in ROWS_PATH)
    assert np.allclose(streamed[0], resident[0], rtol=1e-12, atol=0)


# ------------------------------------------------------------------ 8. two ranks
def test_two_ranks_match_one(prot, tmp_path):
    data, kmers, _ = prot
    torch.manual_seed(3)
    _, init = ar_funcs.make_ar_func_cnn(LAG, 20, filter_width=FW)
    restart = [np.array(0.1)] + [x.detach().numpy() for x in init]
    np.savez(tmp_path / "restart.npz", **{"p%d" % i: x for i, x in enumerate(restart)})
    out_file = tmp_path / "out.json"
    _launch([os.path.join(ROOT, "tests", "prot_cnn_step_worker.py")],
            {"BEAR_RESTART": str(tmp_path / "restart.npz"), "BEAR_OUT": str(out_file), "BEAR_TABLE": str(tmp_path / "prot.tsv")}, tmp_path)
    got = json.load(open(out_file))
    for train_ar in (False, True):
        want = _train_run(data, len(kmers), train_ar=train_ar, params_restart=restart)
        g = got["ar" if train_ar else "bear"]
        assert g["step_fns"] == "wide"
        assert np.allclose(g["loss"], want[0], rtol=1e-10, atol=0)
        for a, b in zip(g["params"], want[1]):
            assert np.allclose(np.asarray(a), b, rtol=1e-7, atol=1e-10)
