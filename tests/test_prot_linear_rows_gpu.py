"""GPU tests of the linear AR function as rows at the protein alphabet's width (bear_linear_forward_wide_f64 /
bear_linear_backward_wide_f64, kernels_linrows_wide.h): forward against the oracle's width-generic ar_func_linear on a one-hot built
from the codes, backward against the NumPy chain (softmax backward + the einsum's transpose), the autograd surface of
make_ar_func_linear(lag, 20) and a captured training step.  Tolerances are those of test_linear_rows_gpu.py: rows 1e-13 relative,
d/d mat 1e-11 of the gradient's largest entry (the NumPy oracle itself is within 2.1e-15 / 8.2e-16 of a long-double evaluation on
these shapes).  The backward pass has no floating-point atomics: repeated launches are held to equal bytes."""
import numpy as np
import pytest
import torch

import bear_oracle as o
from bear_amd import _lib, _train, ar_funcs, bear_net, bear_ref, dataloader, kernels
from test_prot_cpu import make_prot_table, write_prot_tsv

pytestmark = pytest.mark.gpu

W = 21
ROW_RTOL = 1e-13
GRAD_RTOL = 1e-11
MAX_LAG = kernels.LINEAR_WIDE_MAX_LAG
FWD_TILE = 512      # LNW_FWD_TILE
BWD_TILE = 128      # LNW_BWD_TILE
GRID_CAP = "more contexts than the capped grids of both kernels hold tiles: a block takes more than one"


def _codes(n, lag, rng, sorted_rows=False):
    codes = rng.integers(0, 20, size=(n, lag)).astype(np.int8)
    if sorted_rows:         # as a k-mer-ordered batch holds them: first letter most significant
        codes = codes[np.lexsort(codes.T[::-1])]
    codes[rng.random((n, lag)) < 0.03] = 20       # start symbol
    codes[rng.random((n, lag)) < 0.02] = -1       # unknown letter: all-zero one-hot row
    return np.ascontiguousarray(codes)


def _onehot(codes):
    n, lag = codes.shape
    oh = np.zeros((n, lag, W))
    for l in range(lag):
        ok = codes[:, l] >= 0
        oh[np.nonzero(ok)[0], l, codes[ok, l]] = 1.0
    return oh


def _q(n, rng):
    q = rng.normal(size=(n, W)) * np.exp(rng.normal(size=(n, 1)))
    q[rng.random(n) < 0.3] = 0.0                  # contexts without counts: zero gradient rows
    return q


def _want_grad(oh, f, q):
    return np.einsum("njk,nl->jkl", oh, f * (q - (f * q).sum(-1, keepdims=True)))


def _dev(a):
    return torch.from_numpy(a).cuda()


CASES = [(1, 1), (1, 70), (2, 64), (3, 65), (5, 1365), (12, 4097), (MAX_LAG, 257),
         (4, FWD_TILE - 1), (6, FWD_TILE + 1), (7, BWD_TILE - 1), (9, BWD_TILE + 1), (3, GRID_CAP)]


@pytest.mark.parametrize("lag,n", CASES, ids=lambda v: "cap" if v is GRID_CAP else str(v))
@pytest.mark.parametrize("sorted_rows", [False, True])
def test_rows_and_gradient_match_oracle(lag, n, sorted_rows):
    if n is GRID_CAP:       # forward: one block of FWD_TILE per CU; backward: two of BWD_TILE
        n = torch.cuda.get_device_properties(0).multi_processor_count * FWD_TILE + 5 * BWD_TILE + 77
    rng = np.random.default_rng(lag * 1000 + n)
    codes = _codes(n, lag, rng, sorted_rows)
    mat = rng.normal(size=(lag, W, W)) * 0.4
    q = _q(n, rng)
    oh = _onehot(codes)
    want = o.ar_func_linear(oh, mat)
    d_codes = _dev(codes)
    prior = kernels.linear_forward_wide(d_codes, _dev(mat), lag)
    got = prior.cpu().numpy()
    assert got.shape == (n, W)
    assert np.allclose(got, want, rtol=ROW_RTOL, atol=0), np.abs(got / want - 1).max()
    want_g = _want_grad(oh, want, q)
    g = kernels.linear_backward_wide(d_codes, lag, prior, _dev(q)).cpu().numpy()
    assert g.shape == (lag, W, W)
    assert np.abs(g - want_g).max() <= GRAD_RTOL * max(np.abs(want_g).max(), 1e-300), np.abs(g - want_g).max() / np.abs(want_g).max()


def test_edge_rows():
    rng = np.random.default_rng(3)
    n, lag = 1000, 6
    codes = _codes(n, lag, rng)
    codes[codes == 7] = 8               # letter 7 never occurs
    codes[:, 2][codes[:, 2] == 20] = 0  # nor the start symbol at position 2
    codes[100:110] = -1                 # contexts of unknown letters only
    codes[515] = -1
    mat = rng.normal(size=(lag, W, W)) * 0.4
    q = _q(n, rng)
    q[105] = rng.normal(size=W)         # an all-unknown context WITH a gradient row
    d_codes = _dev(codes)
    prior = kernels.linear_forward_wide(d_codes, _dev(mat), lag)
    got = prior.cpu().numpy()
    assert np.abs(got[100:110] - 1.0 / W).max() <= 1e-15 and np.abs(got[515] - 1.0 / W).max() <= 1e-15
    g = kernels.linear_backward_wide(d_codes, lag, prior, _dev(q)).cpu().numpy()
    # the all-unknown contexts contribute to no entry: the gradient without them is the same, and matches the oracle
    keep = np.ones(n, dtype=bool)
    keep[100:110] = keep[515] = False
    want_g = _want_grad(_onehot(codes[keep]), got[keep], q[keep])
    top = np.abs(want_g).max()
    assert np.abs(g - want_g).max() <= GRAD_RTOL * top
    assert np.all(g[:, 7, :] == 0.0) and np.all(g[2, 20, :] == 0.0)          # letters that never occur: exactly zero
    assert np.abs(g.sum(-1)).max() <= 1e-9 * top                             # softmax backward: every row sums to zero
    z = kernels.linear_backward_wide(d_codes, lag, prior, torch.zeros_like(prior)).cpu().numpy()
    assert np.all(z == 0.0)                                                  # no counts anywhere: exact zeros


def test_saturated_logits():
    """Logits of tens, hundreds and thousands: the max-shifted softmax keeps every row finite."""
    rng = np.random.default_rng(5)
    n, lag = 3001, 5
    codes = _codes(n, lag, rng)
    d_codes = _dev(codes)
    oh = _onehot(codes)
    for scale in (8.0, 25.0, 150.0, 400.0, 3000.0):
        mat = rng.normal(size=(lag, W, W)) * 0.4 * scale
        want = o.ar_func_linear(oh, mat)
        got = kernels.linear_forward_wide(d_codes, _dev(mat), lag).cpu().numpy()
        assert np.all(np.isfinite(got)), scale
        if scale <= 150.0:
            big = want > 1e-300
            assert np.abs(got[big] / want[big] - 1).max() <= 1e-11, scale
        else:       # the relative error of tiny entries grows with |logit| eps in the oracle itself
            assert np.abs(got.sum(-1) - 1).max() <= 1e-13, scale
            assert np.abs(got - want).max() <= 1e-13, scale


def test_bit_reproducible():
    rng = np.random.default_rng(8)
    lag, n = 12, 20_011
    d_codes = _dev(_codes(n, lag, rng))
    mat = _dev(rng.normal(size=(lag, W, W)) * 0.4)
    q = _dev(_q(n, rng))
    f1 = kernels.linear_forward_wide(d_codes, mat, lag)
    f2 = kernels.linear_forward_wide(d_codes, mat, lag)
    assert f1.cpu().numpy().tobytes() == f2.cpu().numpy().tobytes()
    g1 = kernels.linear_backward_wide(d_codes, lag, f1, q)
    g2 = kernels.linear_backward_wide(d_codes, lag, f1, q)
    assert float(g1.abs().max()) > 0
    assert g1.cpu().numpy().tobytes() == g2.cpu().numpy().tobytes()


def test_autograd_surface():
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    n, lag = 5000, 7
    codes = _dev(_codes(n, lag, rng))
    onehot = _dev(_onehot(codes.cpu().numpy()))
    gen = torch.Generator(device=dev).manual_seed(3)
    f, (mat,) = ar_funcs.make_ar_func_linear(lag, 20, device=dev, generator=gen)
    assert f.fused
    w = torch.randn(n, W, dtype=torch.float64, device=dev, generator=gen)
    y = f(codes)
    y.backward(w)
    got_y, got_g = y.detach().clone(), mat.grad.clone()
    mat.grad = None
    y2 = f(onehot)                      # the torch formulation
    y2.backward(w)
    assert torch.allclose(got_y, y2.detach(), rtol=ROW_RTOL, atol=0)
    assert float((got_g - mat.grad).abs().max()) <= GRAD_RTOL * float(mat.grad.abs().max())
    with torch.no_grad():               # leading dimensions; nothing is saved
        y3 = f(codes.reshape(50, 100, lag))
    assert y3.shape == (50, 100, W) and y3.grad_fn is None and torch.equal(y3.reshape(n, W), got_y)
    # a lag beyond the kernels' keeps the torch formulation
    long_lag = MAX_LAG + 1
    f2, (mat2,) = ar_funcs.make_ar_func_linear(long_lag, 20, device=dev, generator=gen)
    assert f2.fused is False
    c2 = _codes(300, long_lag, rng)
    want = o.ar_func_linear(_onehot(c2), mat2.detach().cpu().numpy())
    with torch.no_grad():
        assert np.allclose(f2(_dev(c2)).cpu().numpy(), want, rtol=ROW_RTOL, atol=0)


def _torch_formulation(lag, alphabet_size, **kw):
    """make_ar_func_linear with its ar_func held to the one-hot (einsum + softmax) path."""
    f, params = ar_funcs.make_ar_func_linear(lag, alphabet_size, **kw)

    def ar_func(codes):
        oh = torch.nn.functional.one_hot(codes.long() + 1, alphabet_size + 2)[..., 1:]      # -1: an all-zero row
        return f(oh.to(params[0].dtype))
    ar_func.normalized_rows = True
    return ar_func, params


def test_inside_a_captured_step(tmp_path, monkeypatch):
    """A protein table trains through run_autograd_steps with the HIP rows on both sides of dm_prior_wide: the replayed graph and the
    eager loop end in the same bytes (the fixed-order backward), and in the losses of the torch formulation to 1e-9."""
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
        make = _torch_formulation if mode == "torch" else ar_funcs.make_ar_func_linear
        params, _, f = bear_net.train(data.repeat(6), len(kmers), 6, 0, "prot", 4, make, {}, 0.01, "Adam", False, loss_save=losses)
        assert _train.LAST_RUN["graph"] == (mode == "graph")
        if mode != "torch":
            assert f.fused
        runs[mode] = (np.array(losses), [p.detach().cpu().numpy() for p in params])
    assert len(runs["graph"][0]) == 18
    assert runs["graph"][0].tobytes() == runs["eager"][0].tobytes()
    for a, b in zip(runs["graph"][1], runs["eager"][1]):
        assert a.tobytes() == b.tobytes()
    assert np.allclose(runs["graph"][0], runs["torch"][0], rtol=1e-9, atol=0)


def test_bear_ref_with_the_linear_net_function(tmp_path):
    """bear_ref on a protein table mixes the linear net function's rows with the reference prior in torch ops: the HIP rows give the
    losses of the torch formulation (batches stay in table order: the k-mer sort is the 4-letter kernels')."""
    kmers, counts = make_prot_table(seed=0, n=400, num_ds=3)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    data = dataloader.dataloader(str(path), "prot", 150, 3)
    runs = []
    for make in (ar_funcs.make_ar_func_linear, _torch_formulation):
        torch.manual_seed(1)
        losses = []
        bear_ref.train(data.repeat(4), len(kmers), 4, 0, 2, "prot", 4, make, {}, 0.01, "Adam", False, loss_save=losses)
        runs.append(np.array(losses))
    assert len(runs[0]) == 12 and np.allclose(runs[0], runs[1], rtol=1e-9, atol=0)


def test_arguments():
    dev = torch.device("cuda", 0)
    codes = torch.zeros((10, 5), dtype=torch.int8, device=dev)
    mat = torch.zeros((5, W, W), dtype=torch.float64, device=dev)
    rows = torch.full((10, W), 1.0 / W, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        kernels.linear_forward_wide(codes, mat[:4], 5)                       # wrong mat shape
    with pytest.raises(ValueError):
        kernels.linear_backward_wide(codes, 5, rows[:9], rows)               # row-count mismatch
    with pytest.raises(ValueError):
        kernels.linear_forward_wide(codes.to(torch.int32), mat, 5)           # codes are int8
    ws = kernels.default_workspace(dev)
    L, p = _lib.lib(), kernels._ptr
    out = torch.empty((10, W), dtype=torch.float64, device=dev)
    assert L.bear_linear_forward_wide_f64(ws.handle, p(codes), 10, 5, 5, p(mat), p(out), None) == -1          # width 5
    grad = torch.empty((5, W, W), dtype=torch.float64, device=dev)
    assert L.bear_linear_backward_wide_f64(ws.handle, p(codes), 10, 5, 5, p(rows), p(rows), p(grad), None) == -1
    big = MAX_LAG + 1
    c2 = torch.zeros((10, big), dtype=torch.int8, device=dev)
    m2 = torch.zeros((big, W, W), dtype=torch.float64, device=dev)
    assert L.bear_linear_forward_wide_f64(ws.handle, p(c2), 10, big, W, p(m2), p(out), None) == -1             # BEAR_ERR_INVALID_ARG
    with pytest.raises(_lib.BearError):
        kernels.linear_backward_wide(c2, big, rows, rows)
    assert L.bear_linear_forward_wide_f64(ws.handle, p(codes), 10, 0, W, p(mat), p(out), None) == -1
    # an empty batch: no launch, zero gradient
    empty = torch.zeros((0, 5), dtype=torch.int8, device=dev)
    assert kernels.linear_forward_wide(empty, mat, 5).shape == (0, W)
    g = kernels.linear_backward_wide(empty, 5, rows[:0], rows[:0])
    assert g.shape == (5, W, W) and float(g.abs().max()) == 0.0
