"""GPU tests of the convolutional AR function as rows at the protein alphabet's width (bear_cnn_forward_wide_f64 /
bear_cnn_backward_wide_f64, kernels_cnn_wide.h): forward against the oracle's width-generic ar_func_cnn on a one-hot built from the
codes, backward against torch fp64 autograd of make_ar_func_cnn's one-hot path on the device, the autograd surface of
make_ar_func_cnn(lag, 20) and a captured training step.  Tolerances are those of test_cnn_gpu.py: rows 1e-12 relative, each parameter
tensor's gradient within 1e-10 of that tensor's largest entry (at width 21 the NumPy oracle and the two torch formulations agree with
one another to 3.4e-15 on rows and 1.5e-15 on gradients).  The backward pass has no floating-point atomics: repeated launches are held
to equal bytes."""
import numpy as np
import pytest
import torch

import bear_oracle as o
from bear_amd import _lib, _train, ar_funcs, bear_net, bear_ref, dataloader, kernels
from test_prot_cpu import make_prot_table, write_prot_tsv
from test_prot_linear_rows_gpu import _codes, _dev, _onehot, _q

pytestmark = pytest.mark.gpu

W = 21
ROW_RTOL = 1e-12
GRAD_RTOL = 1e-10
MAX_LAG = kernels.CNN_WIDE_MAX_LAG
FWD_TILE = 256      # CNW_FWD_TILE
BWD_TILE = 64       # CNW_BWD_TILE
GRID_CAP = "more contexts than the capped grids of both kernels hold tiles: a block takes more than one"


def _make(lag, fw, seed, **kw):
    """make_ar_func_cnn at the protein alphabet with every parameter moved off its initial value (ones / zeros)."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    ar_func, params = ar_funcs.make_ar_func_cnn(lag, 20, filter_width=fw, device=dev, generator=g, **kw)
    with torch.no_grad():
        for p in params:
            p.add_(0.3 * torch.randn(p.shape, dtype=p.dtype, device=dev, generator=g))
    return ar_func, params


def _flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params]).contiguous()


def _np(params):
    return [p.detach().cpu().numpy() for p in params]


def _autograd_reference(ar_func, params, onehot, grad_rows):
    """d L / d params (flat) through the torch one-hot formulation on the device."""
    for p in params:
        p.grad = None
    rows = ar_func(onehot)
    rows.backward(grad_rows)
    want = torch.cat([p.grad.reshape(-1) for p in params])
    for p in params:
        p.grad = None
    return rows.detach(), want


def _assert_grads(got, want, params, what=""):
    k = 0
    for i, p in enumerate(params):
        m = p.numel()
        err = (got[k:k + m] - want[k:k + m]).abs().max().item()
        top = max(want[k:k + m].abs().max().item(), 1e-300)
        assert err <= GRAD_RTOL * top, (what, i, tuple(p.shape), err / top)
        k += m


CASES = [(1, 1, 1), (1, 1, 70), (4, 1, 64), (5, 3, 65), (8, 8, 130), (12, 8, 1365), (16, 8, 257), (16, 16, 65),
         (6, 4, FWD_TILE - 1), (6, 4, FWD_TILE + 1), (6, 4, BWD_TILE - 1), (6, 4, BWD_TILE + 1), (3, 2, GRID_CAP)]


@pytest.mark.parametrize("lag,fw,n", CASES, ids=lambda v: "cap" if v is GRID_CAP else str(v))
@pytest.mark.parametrize("sorted_rows", [False, True])
def test_rows_and_gradients(lag, fw, n, sorted_rows):
    if n is GRID_CAP:       # forward: at most two blocks of FWD_TILE per CU; backward: one of BWD_TILE
        n = torch.cuda.get_device_properties(0).multi_processor_count * 2 * FWD_TILE + 5 * BWD_TILE + 77
    rng = np.random.default_rng(lag * 1000 + fw * 100 + n)
    codes = _codes(n, lag, rng, sorted_rows)
    ar_func, params = _make(lag, fw, 3)
    flat = _flat(params)
    assert flat.numel() == kernels.cnn_param_count_wide(lag, fw)
    oh = _onehot(codes)
    want = o.ar_func_cnn(oh, _np(params))
    d_codes = _dev(codes)
    prior, t1 = kernels.cnn_forward_wide(d_codes, flat, lag, fw)
    got = prior.cpu().numpy()
    assert got.shape == (n, W) and t1.shape == (n, 16)
    assert np.allclose(got, want, rtol=ROW_RTOL, atol=1e-300), np.abs(got / want - 1).max()
    rows_only, none = kernels.cnn_forward_wide(d_codes, flat, lag, fw, save=False)
    assert none is None and torch.equal(rows_only, prior)
    q = _dev(_q(n, rng))
    g = kernels.cnn_backward_wide(d_codes, flat, lag, fw, t1, prior, q)
    assert g.shape == flat.shape
    _, want_g = _autograd_reference(ar_func, params, _dev(oh), q)
    _assert_grads(g, want_g, params)


@pytest.mark.parametrize("lag,fw", [(6, 3), (6, 6)])
def test_edge_rows(lag, fw):
    rng = np.random.default_rng(3)
    n = 1000
    codes = _codes(n, lag, rng)
    codes[codes == 7] = 8               # letter 7 never occurs
    codes[:, 2][codes[:, 2] == 20] = 0  # nor the start symbol at position 2
    codes[100:110] = -1                 # contexts of unknown letters only
    codes[515] = -1
    ar_func, params = _make(lag, fw, 5)
    flat = _flat(params)
    q = _q(n, rng)
    q[105] = rng.normal(size=W)         # an all-unknown context WITH a gradient row
    q[103] = 0.0                        # ... and one without
    oh = _onehot(codes)
    d_codes, d_q = _dev(codes), _dev(q)
    prior, t1 = kernels.cnn_forward_wide(d_codes, flat, lag, fw)
    want = o.ar_func_cnn(oh, _np(params))
    got = prior.cpu().numpy()
    assert np.allclose(got, want, rtol=ROW_RTOL, atol=1e-300)
    assert np.all(got[100:110] == got[515])                                  # conv = 0 in all of them: one and the same row
    g = kernels.cnn_backward_wide(d_codes, flat, lag, fw, t1, prior, d_q)
    _, want_g = _autograd_reference(ar_func, params, _dev(oh), d_q)
    _assert_grads(g, want_g, params)
    gf = g[:fw * W * 30].reshape(fw, W, 30).cpu().numpy()
    assert np.abs(gf).max() > 0
    assert np.all(gf[:, 7, :] == 0.0)                                        # a letter that never occurs: exactly zero
    if fw == lag:                       # one position: tap 2 reads letter 2 of the context, which is never the start symbol
        assert np.all(gf[2, 20, :] == 0.0)
    z = kernels.cnn_backward_wide(d_codes, flat, lag, fw, t1, prior, torch.zeros_like(prior))
    assert np.all(z.cpu().numpy() == 0.0)                                    # no counts anywhere: exact zeros
    # an empty batch: shapes, a zero gradient
    empty = torch.zeros((0, lag), dtype=torch.int8, device=d_codes.device)
    p0, t0 = kernels.cnn_forward_wide(empty, flat, lag, fw)
    assert p0.shape == (0, W) and t0.shape == (0, 16)
    g0 = kernels.cnn_backward_wide(empty, flat, lag, fw, t0, p0, p0)
    assert g0.shape == flat.shape and float(g0.abs().max()) == 0.0


def test_bit_reproducible():
    rng = np.random.default_rng(8)
    lag, fw, n = 12, 8, 20_011
    d_codes = _dev(_codes(n, lag, rng))
    flat = _flat(_make(lag, fw, 7)[1])
    q = _dev(_q(n, rng))
    f1, t1 = kernels.cnn_forward_wide(d_codes, flat, lag, fw)
    f2, t2 = kernels.cnn_forward_wide(d_codes, flat, lag, fw)
    assert f1.cpu().numpy().tobytes() == f2.cpu().numpy().tobytes() and t1.cpu().numpy().tobytes() == t2.cpu().numpy().tobytes()
    g1 = kernels.cnn_backward_wide(d_codes, flat, lag, fw, t1, f1, q)
    g2 = kernels.cnn_backward_wide(d_codes, flat, lag, fw, t1, f1, q)
    assert float(g1.abs().max()) > 0
    assert g1.cpu().numpy().tobytes() == g2.cpu().numpy().tobytes()


def test_autograd_surface():
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    n, lag, fw = 5000, 7, 4
    codes = _dev(_codes(n, lag, rng))
    onehot = _dev(_onehot(codes.cpu().numpy()))
    f, params = _make(lag, fw, 3)
    assert f.fused
    gen = torch.Generator(device=dev).manual_seed(4)
    w = torch.randn(n, W, dtype=torch.float64, device=dev, generator=gen)
    y = f(codes)
    assert y.grad_fn is not None
    y.backward(w)
    got_y, got_g = y.detach().clone(), torch.cat([p.grad.reshape(-1) for p in params])
    want_y, want_g = _autograd_reference(f, params, onehot, w)       # the torch formulation
    assert torch.allclose(got_y, want_y, rtol=ROW_RTOL, atol=1e-300)
    _assert_grads(got_g, want_g, params)
    with torch.no_grad():               # leading dimensions; nothing is saved
        y3 = f(codes.reshape(50, 100, lag))
    assert y3.shape == (50, 100, W) and y3.grad_fn is None and torch.equal(y3.reshape(n, W), got_y)
    # shapes beyond the kernels' keep the torch formulation
    for long_lag, kw in ((MAX_LAG + 1, {}), (9, {"num_filters": 20})):
        f2, p2 = _make(long_lag, 5, 6, **kw)
        assert f2.fused is False
        c2 = _codes(300, long_lag, rng)
        want = o.ar_func_cnn(_onehot(c2), _np(p2))
        with torch.no_grad():
            assert np.allclose(f2(_dev(c2)).cpu().numpy(), want, rtol=ROW_RTOL, atol=1e-300)


def _torch_formulation(lag, alphabet_size, **kw):
    """make_ar_func_cnn with its ar_func held to the one-hot (conv1d) path."""
    f, params = ar_funcs.make_ar_func_cnn(lag, alphabet_size, **kw)

    def ar_func(codes):
        oh = torch.nn.functional.one_hot(codes.long() + 1, alphabet_size + 2)[..., 1:]      # -1: an all-zero row
        return f(oh.to(params[0].dtype))
    ar_func.normalized_rows = True
    return ar_func, params


def test_inside_a_captured_step(tmp_path, monkeypatch):
    """A protein table trains through run_autograd_steps with the HIP rows on both sides of dm_prior_wide: the replayed graph and the
    eager loop end in the same bytes (the fixed-order backward), and in the losses of the torch formulation to 1e-9 (a check of the
    wiring: a relative row error of 1e-6 moves a loss by 4e-9; the tests above guard the rounding)."""
    kmers, counts = make_prot_table(seed=0, n=400, num_ds=3)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    data = dataloader.dataloader(str(path), "prot", 150, 3)
    runs = {}
    for mode in ("graph", "eager", "torch"):
        if mode != "graph":
            monkeypatch.setenv("BEAR_AMD_GRAPH_MAX_ROWS", "0")
        torch.manual_seed(1)
        losses = []
        make = _torch_formulation if mode == "torch" else ar_funcs.make_ar_func_cnn
        params, _, f = bear_net.train(data.repeat(6), len(kmers), 6, 0, "prot", 4, make, {"filter_width": 3}, 0.01, "Adam", False,
                                      loss_save=losses)
        assert _train.LAST_RUN["graph"] == (mode == "graph")
        if mode != "torch":
            assert f.fused
        runs[mode] = (np.array(losses), [p.detach().cpu().numpy() for p in params])
    assert len(runs["graph"][0]) == 18
    assert runs["graph"][0].tobytes() == runs["eager"][0].tobytes()
    for a, b in zip(runs["graph"][1], runs["eager"][1]):
        assert a.tobytes() == b.tobytes()
    assert np.allclose(runs["graph"][0], runs["torch"][0], rtol=1e-9, atol=0)


def test_bear_ref_with_the_cnn_net_function(tmp_path):
    """bear_ref on a protein table mixes the cnn net function's rows with the reference prior in torch ops: the HIP rows give the
    losses of the torch formulation."""
    kmers, counts = make_prot_table(seed=0, n=400, num_ds=3)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    data = dataloader.dataloader(str(path), "prot", 150, 3)
    runs = []
    for make in (ar_funcs.make_ar_func_cnn, _torch_formulation):
        torch.manual_seed(1)
        losses = []
        bear_ref.train(data.repeat(4), len(kmers), 4, 0, 2, "prot", 4, make, {"filter_width": 3}, 0.01, "Adam", False, loss_save=losses)
        runs.append(np.array(losses))
    assert len(runs[0]) == 12 and np.allclose(runs[0], runs[1], rtol=1e-9, atol=0)


def test_arguments():
    dev = torch.device("cuda", 0)
    lag, fw = 5, 3
    n_par = kernels.cnn_param_count_wide(lag, fw)
    codes = torch.zeros((10, lag), dtype=torch.int8, device=dev)
    flat = torch.zeros(n_par, dtype=torch.float64, device=dev)
    rows = torch.full((10, W), 1.0 / W, dtype=torch.float64, device=dev)
    t1 = torch.zeros((10, 16), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        kernels.cnn_forward_wide(codes, flat[:-1], lag, fw)                          # wrong parameter count
    with pytest.raises(ValueError):
        kernels.cnn_backward_wide(codes, flat, lag, fw, t1, rows[:9], rows)          # row-count mismatch
    with pytest.raises(ValueError):
        kernels.cnn_backward_wide(codes, flat, lag, fw, t1[:9], rows, rows)
    with pytest.raises(ValueError):
        kernels.cnn_forward_wide(codes.to(torch.int32), flat, lag, fw)               # codes are int8
    with pytest.raises(_lib.BearError):
        kernels.cnn_forward_wide(torch.zeros((10, MAX_LAG + 1), dtype=torch.int8, device=dev), flat, MAX_LAG + 1, fw)
    ws = kernels.default_workspace(dev)
    L, p = _lib.lib(), kernels._ptr
    out = torch.empty((10, W), dtype=torch.float64, device=dev)
    grad = torch.empty(n_par, dtype=torch.float64, device=dev)
    big = torch.zeros((10, MAX_LAG + 1), dtype=torch.int8, device=dev)

    def fwd(c, lag_, fw_, nf, l1, width):
        return L.bear_cnn_forward_wide_f64(ws.handle, p(c), 10, lag_, fw_, nf, l1, width, p(flat), p(out), None, None)

    def bwd(c, lag_, fw_, nf, l1, width):
        return L.bear_cnn_backward_wide_f64(ws.handle, p(c), 10, lag_, fw_, nf, l1, width, p(flat), p(t1), p(rows), p(rows), p(grad), None)

    for call in (fwd, bwd):             # every refused shape: BEAR_ERR_INVALID_ARG, nothing launched
        assert call(codes, lag, fw, 30, 16, 5) == -1                                 # width 5
        assert call(codes, lag, fw, 20, 16, W) == -1                                 # 20 filters
        assert call(codes, lag, fw, 30, 8, W) == -1                                  # layer-1 width 8
        assert call(codes, lag, 0, 30, 16, W) == -1                                  # filter_width < 1
        assert call(codes, lag, lag + 1, 30, 16, W) == -1                            # filter_width > lag
        assert call(big, MAX_LAG + 1, fw, 30, 16, W) == -1                           # lag > CNN_WIDE_MAX_LAG
    assert fwd(codes, lag, fw, 30, 16, W) == 0 and bwd(codes, lag, fw, 30, 16, W) == 0
    torch.cuda.synchronize()
