"""The protein alphabet on the GPU: the width-generic kernels (kernels_wide.h) against the oracle and, at W = 5, against the
trusted 5-wide entry points; training and evaluation of a 21-letter table end to end."""
import configparser
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bear_oracle as o
import c_oracle as co
from bear_amd import _lib, _train, ar_funcs, bear_net, bear_ref, core, dataloader, kernels
from conftest import ROOT, YSD1
from test_prot_cpu import make_prot_table, write_prot_tsv

pytestmark = pytest.mark.gpu
EPS = 1e-7
W = 21


class HashNoiseW(o.HashNoise):
    """HashNoise with the cell key row * width + letter (eval_noise(..., width))."""

    def __init__(self, seed, row_base, n_rows, width):
        super().__init__(seed, row_base, n_rows)
        self.width = width

    def normal(self, model):
        return o.eval_noise(self.seed, model, self.rows, width=self.width)


def keras_adam_np(p, g, m, v, t, lr=0.01, b1=0.9, b2=0.999, eps=1e-7):
    m[...] = b1 * m + (1 - b1) * g
    v[...] = b2 * v + (1 - b2) * g * g
    lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    p[...] = p - lr_t * m / (np.sqrt(v) + eps)


def _dev_counts(c):
    return torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda()


def _priors(rng, n, width, tiny=False):
    z = rng.normal(size=(n, width)) * 2.0
    f = np.exp(z - z.max(1, keepdims=True))
    f /= f.sum(1, keepdims=True)
    if tiny and n:
        f[rng.random((n, width)) < 0.1] = 1e-300           # entries near the bottom of the double range
    return f


def _tables():
    rng = np.random.default_rng(11)
    _, sparse = make_prot_table(seed=5, n=1037)                  # 1037: not a multiple of the tile
    dense = rng.integers(1000, 100_000, (700, W)).astype(np.uint32)
    return {"sparse": sparse[0], "sparse_b": sparse[1], "dense": dense, "one": sparse[0][:1], "empty": sparse[0][:0]}


@pytest.mark.parametrize("table", ["sparse", "sparse_b", "dense", "one", "empty"])
@pytest.mark.parametrize("train_ar", [False, True])
@pytest.mark.parametrize("want_grad", [False, True])
def test_dm_prior_wide_matches_oracle(table, train_ar, want_grad):
    c = _tables()[table]
    rng = np.random.default_rng(len(c) + 7)
    f = _priors(rng, len(c), W, tiny=table != "dense")
    h_signed = 0.37
    h_dev = torch.tensor([h_signed], dtype=torch.float64, device="cuda")
    out, grad = kernels.dm_prior_wide(_dev_counts(c), torch.from_numpy(f).cuda(), h_dev, train_ar=train_ar, want_grad=want_grad)
    got = out.cpu().numpy()
    if not len(c):
        assert got.tolist() == [0.0, 0.0] and (grad is None or grad.shape == (0, W))
        return
    want = o.bear_net_step(c, f, h_signed, train_ar=train_ar)
    assert np.isclose(got[0], want["ll"], rtol=1e-11, atol=0), (got[0], want["ll"])
    if train_ar:
        assert got[1] == 0.0
    else:
        h = np.exp(h_signed)
        terms = o.dm_grad_concentration(f / h + EPS, c) * (-f / h)
        assert abs(got[1] - want["d_h_signed"]) <= 2e-13 * np.abs(terms).sum()
    if want_grad:
        g = grad.cpu().numpy()
        assert g.shape == c.shape
        assert np.abs(g - want["d_prior"]).max() <= 2e-13 * np.abs(want["d_prior"]).sum()
        # and every entry within 1e-12 of its own mass (AR mode: relative), against the width-generic C oracle
        _, wg = co.dm_prior_w(c, f, h_signed, train_ar=train_ar, want_grad=True)
        _, gm = co.dm_prior_mass_w(c, f, h_signed, train_ar=train_ar, want_grad=True)
        assert (np.abs(g - wg) <= 1e-12 * (np.abs(wg) if train_ar else gm)).all()
        assert (g[c.sum(1) == 0] == 0).all()
    else:
        assert grad is None


@pytest.mark.parametrize("train_ar", [False, True])
def test_wide_kernels_at_width_5_match_the_5_wide_entry_points(train_ar, ysd1):
    _, counts = ysd1
    c = counts[:, 0].astype(np.uint32)
    rng = np.random.default_rng(2)
    f = _priors(rng, len(c), 5, tiny=True)
    cd, fd = _dev_counts(c), torch.from_numpy(f).cuda()
    h_dev = torch.tensor([-0.4], dtype=torch.float64, device="cuda")
    for want_grad in (False, True):
        ref, gref = kernels.dm_prior(cd, fd, -0.4, train_ar=train_ar, want_grad=want_grad)
        got, g = kernels.dm_prior_wide(cd, fd, h_dev, train_ar=train_ar, want_grad=want_grad)
        ref, got = ref.cpu().numpy(), got.cpu().numpy()
        assert np.isclose(got[0], ref[0], rtol=1e-12) and np.isclose(got[1], ref[1], rtol=1e-12, atol=1e-12 * abs(ref[0]))
        if want_grad:
            gw = gref.cpu().numpy()
            assert np.allclose(g.cpu().numpy(), gw, rtol=1e-12, atol=1e-13 * np.abs(gw).max())
    # the evaluation: same sums, the same accuracies exactly (the noise stream is keyed by row * 5 + letter in both)
    test, train = _dev_counts(counts[:, 1].astype(np.uint32)), _dev_counts(c)
    for tr in (train, None):
        want = kernels.evaluate(test, fd, [0.3, 2.0], [0.1, 1.0, 10.0], tr, noise_seed=5, row_base=100).cpu().numpy()
        got = kernels.evaluate_wide(test, fd, [0.3, 2.0], [0.1, 1.0, 10.0], tr, noise_seed=5, row_base=100).cpu().numpy()
        ll = np.r_[0:6]
        assert np.allclose(got[ll], want[ll], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(got[6:], want[6:])


@pytest.mark.parametrize("use_train", [True, False])
def test_evaluate_wide_matches_oracle(use_train):
    _, counts = make_prot_table(seed=9, n=1500, num_ds=2)
    test, train = counts[1], counts[0]
    rng = np.random.default_rng(4)
    f = _priors(rng, len(test), W)
    hs, van = [0.05, 0.4, 3.0], [0.1, 1.0, 10.0]
    got = kernels.evaluate_wide(_dev_counts(test), torch.from_numpy(f).cuda(), hs, van, _dev_counts(train) if use_train else None,
                                noise_seed=3, row_base=77).cpu().numpy()
    w = o.evaluation_step(test, f, np.array(hs), van, train if use_train else None, rng=HashNoiseW(3, 77, len(test), W))
    H, V = len(hs), len(van)
    assert np.allclose(got[:H], w[0], rtol=1e-11, atol=0) and np.isclose(got[H], w[1], rtol=1e-11)
    assert np.allclose(got[H + 1:H + 1 + V], w[2], rtol=1e-11, atol=0)
    np.testing.assert_array_equal(got[H + V + 1:2 * H + V + 1], w[3])
    assert got[2 * H + V + 1] == w[4]
    np.testing.assert_array_equal(got[2 * H + V + 2:2 * H + 2 * V + 2], w[5])
    assert got[-1] == w[6]


def test_bad_width_is_refused():
    L = _lib.lib()
    ws = kernels.default_workspace(torch.device("cuda", 0))
    c = torch.zeros((8, 7), dtype=torch.int32, device="cuda")
    f = torch.zeros((8, 7), dtype=torch.float64, device="cuda")
    h = torch.zeros(1, dtype=torch.float64, device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    p = kernels._ptr
    assert L.bear_dm_prior_wide_f64(ws.handle, p(c), p(f), 8, 7, p(h), EPS, 0, p(out), None, None) == -1
    hv = np.array([1.0])
    assert L.bear_eval_wide_f64(ws.handle, p(c), None, p(f), 8, 7, hv.ctypes.data, 1, 1, None, 0, EPS, 0, 0, p(out), None) == -1
    with pytest.raises(ValueError):
        kernels.dm_prior_wide(c, f, h)


def _prot_data(tmp_path, n=600, batch=250, seed=0, num_ds=3):
    kmers, counts = make_prot_table(seed=seed, n=n, num_ds=num_ds)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    return dataloader.dataloader(str(path), "prot", batch, num_ds), kmers, counts


@pytest.mark.parametrize("name", ["linear", "stop"])
@pytest.mark.parametrize("train_ar", [False, True])
def test_bear_net_train_prot_matches_oracle_loop(name, train_ar, tmp_path):
    data, kmers, counts = _prot_data(tmp_path)
    n, B, epochs = len(kmers), 250, 8
    make = getattr(ar_funcs, "make_ar_func_" + name)
    torch.manual_seed(3)
    _, init = make(4, 20)
    init_np = [x.detach().numpy().copy() for x in init]
    loss_save = []
    params, h_signed, ar_func = bear_net.train(data.repeat(epochs), n, epochs, 0, "prot", 4, make, {}, 0.01, "Adam", train_ar,
                                               params_restart=[np.array(0.1)] + init_np, loss_save=loss_save)
    assert _train.LAST_RUN["graph"]
    f_cpu, p_cpu = make(4, 20)
    with torch.no_grad():
        for a, b in zip(p_cpu, init_np):
            a.copy_(torch.as_tensor(b))
    h = np.array(0.1)
    ms = [np.zeros_like(h)] + [np.zeros(x.shape) for x in p_cpu]
    vs = [np.zeros_like(h)] + [np.zeros(x.shape) for x in p_cpu]
    codes = torch.as_tensor(data.codes())
    c0 = counts[0]
    want_loss, t = [], 0
    for _ in range(epochs):
        for a in range(0, n, B):
            b = min(a + B, n)
            for q in p_cpu:
                q.grad = None
            prior = f_cpu(codes[a:b])
            r = o.bear_net_step(c0[a:b], prior.detach().numpy(), float(h), train_ar=train_ar)
            scale = -(n / (b - a))
            if prior.requires_grad:
                prior.backward(torch.as_tensor(scale * r["d_prior"]))
            want_loss.append(-scale * r["ll"])
            t += 1
            if not train_ar:
                keras_adam_np(h, np.array(scale * r["d_h_signed"]), ms[0], vs[0], t)
            for i, q in enumerate(p_cpu):
                keras_adam_np(q.detach().numpy(), q.grad.numpy(), ms[i + 1], vs[i + 1], t)
    assert len(loss_save) == len(want_loss) == 24
    assert np.allclose(loss_save, want_loss, rtol=1e-9)
    assert np.isclose(params[0].item(), float(h), rtol=1e-7, atol=1e-9)
    for got, want in zip(params[1:], p_cpu):
        assert np.allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("train_ar", [False, True])
def test_bear_ref_train_prot_stop_matches_oracle_loop(train_ar, tmp_path):
    data, kmers, counts = _prot_data(tmp_path)
    n, B, epochs = len(kmers), 250, 8
    loss_save = []
    params, _, ar_func = bear_ref.train(data.repeat(epochs), n, epochs, 0, 2, "prot", 4, ar_funcs.make_ar_func_stop, {}, 0.01, "Adam",
                                        train_ar, loss_save=loss_save)
    p = np.array([0.0, np.log(1 / 30), -np.log(100)])
    m, v = np.zeros(3), np.zeros(3)
    want_loss, t = [], 0
    for _ in range(epochs):
        for a in range(0, n, B):
            b = min(a + B, n)
            r = o.bear_ref_step(counts[0, a:b], counts[2, a:b], *p, train_ar=train_ar)
            scale = -(n / (b - a))
            want_loss.append(-scale * r["ll"])
            g = scale * np.array([r["d_h_signed"], r["d_tau_signed"], r["d_nu_signed"]])
            t += 1
            if train_ar:
                keras_adam_np(p[1:], g[1:], m[1:], v[1:], t)
            else:
                keras_adam_np(p, g, m, v, t)
    assert np.allclose(loss_save, want_loss, rtol=1e-9)
    assert np.allclose([x.item() for x in params], p, rtol=1e-7, atol=1e-9)


def test_graph_replay_equals_eager(tmp_path, monkeypatch):
    data, kmers, _ = _prot_data(tmp_path, n=400, batch=150)
    runs = {}
    for mode in ("graph", "eager"):
        if mode == "eager":
            monkeypatch.setenv("BEAR_AMD_GRAPH_MAX_ROWS", "0")
        torch.manual_seed(1)
        losses = []
        params, _, _ = bear_net.train(data.repeat(6), len(kmers), 6, 0, "prot", 4, ar_funcs.make_ar_func_linear, {}, 0.01, "Adam", False,
                                      loss_save=losses)
        assert _train.LAST_RUN["graph"] == (mode == "graph")
        runs[mode] = (np.array(losses), [q.detach().cpu().numpy() for q in params])
    assert np.allclose(runs["graph"][0], runs["eager"][0], rtol=1e-13, atol=0)
    for a, b in zip(runs["graph"][1], runs["eager"][1]):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-15)


def test_evaluation_prot_matches_oracle(tmp_path):
    """End to end: the AR rows come from torch ops here and from NumPy in the oracle (they agree to the last bits, not bit for bit),
    so the log-likelihoods are held to 1e-9; the kernel's own precision is pinned by test_evaluate_wide_matches_oracle (1e-11)."""
    rtol = 1e-9
    data, kmers, counts = _prot_data(tmp_path, n=800, batch=300)
    torch.manual_seed(2)
    f, p = ar_funcs.make_ar_func_linear(4, 20, device="cuda")
    prior = o.ar_func_linear(o.one_hot(kmers, "prot"), p[0].detach().cpu().numpy())
    van = np.array([0.1, 1.0, 10.0])
    noise = HashNoiseW(11, 0, len(kmers), W)
    for use_train in (True, False):
        got = bear_net.evaluation(data, 0 if use_train else -1, 1, "prot", torch.tensor(0.37), f, van, seed=11)
        w = o.evaluation_step(counts[1], prior, 0.37, van, counts[0] if use_train else None, rng=noise)
        total = w[6]
        assert np.isclose(got[0], w[0], rtol=rtol) and np.isclose(got[1], w[1], rtol=rtol)
        assert np.allclose(got[2], w[2], rtol=rtol)
        assert np.isclose(got[6], w[3] / total, rtol=0, atol=0) and np.isclose(got[7], w[4] / total, rtol=0, atol=0)
        np.testing.assert_array_equal(got[8], w[5] / total)
    hs = np.array([0.1, 0.37, 4.0])
    ll, perp, acc = bear_net.h_scan(data, 0, 1, "prot", torch.tensor(hs), f, seed=11)
    w = o.evaluation_step(counts[1], prior, hs, np.ones(1), counts[0], rng=noise)
    assert np.allclose(ll, w[0], rtol=rtol) and np.array_equal(acc, w[3] / w[6])
    # bear_ref with the stop net function: prior = the mixture of bear_ref.py:63-68
    torch.manual_seed(0)
    params_r, ar_r = bear_ref._create_params(4, 20, ar_funcs.make_ar_func_stop, {}, device="cuda")[::2]
    tau_s, nu_s = params_r[1].item(), params_r[2].item()
    got = bear_ref.evaluation(data, 0, 1, 2, "prot", torch.tensor(0.5), ar_r, van, seed=4)
    prior_r = o.ref_ar_func(o.ar_func_stop(None, 20), o.ref_input(counts[2]), tau_s, nu_s)
    w = o.evaluation_step(counts[1], prior_r, 0.5, van, counts[0], rng=HashNoiseW(4, 0, len(kmers), W))
    assert np.isclose(got[0], w[0], rtol=rtol) and np.isclose(got[1], w[1], rtol=rtol) and np.allclose(got[2], w[2], rtol=rtol)
    assert got[6] == w[3] / w[6] and got[7] == w[4] / w[6]


@pytest.mark.parametrize("kind", ["net", "ref"])
def test_driver_runs_a_prot_config(kind, tmp_path):
    from bear_amd.models import train_bear_net, train_bear_ref
    kmers, counts = make_prot_table(seed=1, n=500, num_ds=3)
    (tmp_path / "in").mkdir()
    write_prot_tsv(tmp_path / "in" / "protk4.tsv", kmers, counts)
    config = configparser.ConfigParser()
    config.read(os.path.join(ROOT, "bear_amd", "models", "config_files", "bear_test.cfg"))
    config["general"]["out_folder"] = str(tmp_path / "out") + "*"
    config["data"].update({"files_path": str(tmp_path / "in"), "start_token": "protk", "alphabet": "prot"})
    config["hyperp"]["lag"] = "4"
    config["train"].update({"batch_size": "200", "epochs": "3", "train_ar": "False"})
    if kind == "ref":
        config["model"]["ar_func_name"] = "stop"
    mod = train_bear_net if kind == "net" else train_bear_ref
    exit_code, ll_van, perp_van = mod.main(config)
    assert exit_code == 1 and np.isfinite(ll_van).all() and np.isfinite(perp_van).all()
    for key in ("heldout_loglikelihood_BEAR", "heldout_perplex_AR", "heldout_accuracy_BEAR", "h"):
        assert np.isfinite(float(config["results"][key]))


def test_deterministic_build_wide_step_is_bit_reproducible(tmp_path):
    script = tmp_path / "det_wide.py"
    script.write_text(
        "import sys\nsys.path.insert(0, sys.argv[1])\nsys.path.insert(0, sys.argv[1] + '/tests')\n"
        "import numpy as np, torch\nfrom bear_amd import _lib, kernels\nfrom test_prot_cpu import make_prot_table\n"
        "assert _lib.lib().bear_deterministic_build() == 1, _lib.LIB_PATH\n"
        "_, c = make_prot_table(seed=2, n=20000, num_ds=1)\n"
        "cd = torch.from_numpy(c[0].view(np.int32)).cuda()\n"
        "z = np.random.default_rng(0).random((20000, 21)); f = torch.from_numpy(z / z.sum(1, keepdims=True)).cuda()\n"
        "h = torch.tensor([0.2], dtype=torch.float64, device='cuda')\n"
        "a = [x.cpu().numpy().tobytes() for x in kernels.dm_prior_wide(cd, f, h, want_grad=True)]\n"
        "b = [x.cpu().numpy().tobytes() for x in kernels.dm_prior_wide(cd, f, h, want_grad=True)]\n"
        "assert a == b\nprint('DET_WIDE_OK')\n")
    env = dict(os.environ, BEAR_AMD_DETERMINISTIC="1")
    env.pop("BEAR_AMD_LIB", None)
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "DET_WIDE_OK" in p.stdout, p.stdout + p.stderr
