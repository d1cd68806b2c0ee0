"""GPU tests of shuffled epochs that do not send whole columns through the device: bear_shuffle_rows_range against
bear_shuffle_rows; the batch entries of a streamed and of a multi-rank shuffled epoch against the resident single-rank ones
(exact); training and evaluation over streamed shuffled batches against the resident shuffled run (the comparison and tolerances
of test_train_gpu.py::test_streamed_epochs_equal_resident_epochs); and the automatic switch to streaming."""
import numpy as np
import pytest
import torch

from bear_amd import _lib, _train, ar_funcs, bear_net, bear_ref, dataloader, dist, kernels
from conftest import YSD1
from test_prot_cpu import make_prot_table, write_prot_tsv

pytestmark = pytest.mark.gpu

SEED = 3
ROW_FORMS = ((5, np.int32), (21, np.int32), (None, np.int64), (13, np.int8))      # rows of 20, 84, 8 and 13 bytes: words, words, words, bytes
# (first, n_out): empty, whole, first > 0 up to n_rows, interior.  The whole range of 70 001 rows of 84 bytes is 1 470 021 words:
# more than the 4096 blocks of 256 threads a launch has at most (SHF_MAX_BLOCKS), so the word kernel strides twice; the byte kernel's
# second trip is test_byte_rows_beyond_one_grid_match_the_oracle_permutation's.
ranges = lambda n: sorted({(0, 0), (n, 0), (n // 2, 0), (0, n), (n - n // 3, n // 3), (n // 4, n // 2), (min(1, n), n - min(1, n))})


def device():
    return torch.device("cuda", torch.cuda.current_device())


def table(n, width, dtype, rng):
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=(n,) if width is None else (n, width), dtype=dtype)


@pytest.fixture(scope="module")
def whole_shuffles():
    """(n, form) -> (host table, shuffle_rows of it on the device): computed once, shared, left unchanged."""
    rng = np.random.default_rng(5)
    out = {}
    for n in (1, 2, 1365, 70_001):
        for width, dtype in ROW_FORMS:
            a = table(n, width, dtype, rng)
            out[(n, width)] = (a, kernels.shuffle_rows(torch.from_numpy(a).to(device()), SEED))
    return out


@pytest.mark.parametrize("n", [1, 2, 1365, 70_001])
def test_range_from_device_memory_equals_slices_of_the_whole_shuffle(n, whole_shuffles):
    assert 70_001 * 21 > 4096 * 256
    for width, _ in ROW_FORMS:
        a, whole = whole_shuffles[(n, width)]
        src = torch.from_numpy(a).to(device())
        for first, n_out in ranges(n):
            got = kernels.shuffle_rows_range(src, first, n_out, SEED)
            assert got.dtype == src.dtype and got.shape == (n_out,) + src.shape[1:]
            assert torch.equal(got, whole[first:first + n_out]), (width, first, n_out)
        # the caller's own destination, and the same bytes described as rows of another shape
        out = torch.empty((n // 2,) + src.shape[1:], dtype=src.dtype, device=src.device)
        assert kernels.shuffle_rows_range(src, n // 4, n // 2, SEED, out=out) is out and torch.equal(out, whole[n // 4:n // 4 + n // 2])
        if width is not None:
            flat = kernels.shuffle_rows_range(src.reshape(-1), n // 4, n // 2, SEED, n_rows=n, row_shape=(width,))
            assert torch.equal(flat, whole[n // 4:n // 4 + n // 2])
            with pytest.raises(ValueError):
                kernels.shuffle_rows_range(src.reshape(-1), 0, 1, SEED, n_rows=n + 1, row_shape=(width,))
    with pytest.raises(ValueError):
        kernels.shuffle_rows_range(src, n, 1, SEED)
    with pytest.raises(ValueError):
        kernels.shuffle_rows_range(src, 0, n + 1, SEED)


def test_byte_rows_beyond_one_grid_match_the_oracle_permutation():
    """90 001 rows of 13 bytes are 1 170 013 bytes: more than the 4096 x 256 threads of a launch, so shuffle_bytes_kernel strides
    twice, whole and by range.  The reference is the oracle's permutation, not the kernel itself."""
    import bear_oracle as o
    n = 90_001
    assert n * 13 > 4096 * 256
    a = table(n, 13, np.int8, np.random.default_rng(13))
    want = a[np.asarray(o.shuffle_perm(n, SEED), dtype=np.int64)]
    src = torch.from_numpy(a).to(device())
    assert np.array_equal(kernels.shuffle_rows(src, SEED).cpu().numpy(), want)
    assert np.array_equal(kernels.shuffle_rows_range(src, 0, n, SEED).cpu().numpy(), want)
    assert np.array_equal(kernels.shuffle_rows_range(src, 7, n - 8, SEED).cpu().numpy(), want[7:n - 1])
    words = table(70_001, 21, np.int32, np.random.default_rng(21))           # and the word kernel's second trip, likewise
    got = kernels.shuffle_rows_range(torch.from_numpy(words).to(device()), 1, 70_000, SEED).cpu().numpy()
    assert np.array_equal(got, words[np.asarray(o.shuffle_perm(70_001, SEED), dtype=np.int64)][1:])


def test_the_c_entry_refuses_a_range_beyond_the_table():
    import ctypes
    src = torch.zeros(10, 5, dtype=torch.int32, device=device())
    dst = torch.full((12, 5), 7, dtype=torch.int32, device=device())
    L = _lib.lib()
    s, d = ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr())
    for first, n_out in ((0, 11), (5, 6), (10, 1), (11, 0)):
        assert L.bear_shuffle_rows_range(s, d, 10, first, n_out, 20, SEED, None) == -1
    assert L.bear_shuffle_rows_range(s, d, 10, 10, 0, 20, SEED, None) == 0
    torch.cuda.synchronize()
    assert bool((dst == 7).all())


# ------------------------------------------------------------------------------------------------ ResidentBatches
COLUMNS = {"train": 0, "test": 1, "ref": 2}


def ysd1_table():
    data = dataloader.dataloader(YSD1, "dna", 500, 3)           # 1365 rows: three batches, the last one short (365 rows)
    data.counts[0, ::4] = 0
    return data


@pytest.fixture(scope="module")
def prot_table(tmp_path_factory):
    kmers, counts = make_prot_table(seed=4, n=600, num_ds=3)
    path = tmp_path_factory.mktemp("prot") / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    return dataloader.dataloader(str(path), "prot", 250, 3)     # three batches: 250, 250, 100


def build(data, **kw):
    kw = dict(dict(want_codes=True, drop_empty="train", kmer_order=True), **kw)
    return _train.ResidentBatches(data, COLUMNS, device(), **kw)


def snapshot(res):
    """Every batch's entry on the host: meta data, every slab and row_ids (where the entry has them)."""
    out = []
    for k, e in res.loaded():
        out.append({name: (e[name].cpu().numpy() if isinstance(e[name], torch.Tensor) else e[name])
                    for name in ("global_rows", "rows", "row0", "train", "test", "ref", "codes", "row_ids") if name in e})
    res.close()
    return out


def assert_same_entries(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for name in w:
            if isinstance(w[name], np.ndarray):
                assert g[name].dtype == w[name].dtype and np.array_equal(g[name], w[name]), name
            else:
                assert g[name] == w[name], name


@pytest.mark.parametrize("kmer_order", [True, False])
@pytest.mark.parametrize("drop_empty", ["train", None])
def test_streamed_shuffled_entries_equal_the_resident_ones(kmer_order, drop_empty):
    data = ysd1_table().shuffle(3)
    kw = dict(kmer_order=kmer_order, drop_empty=drop_empty)
    resident = build(data, **kw)
    assert resident.streaming is False and resident._by_range is False
    want = snapshot(resident)
    assert [w["global_rows"] for w in want] == [500, 500, 365]
    if drop_empty:
        assert all(w["rows"] < w["global_rows"] for w in want)
    res = build(data, stream=True, **kw)
    assert res.streaming is True and res._by_range is True
    got = [snapshot_one(res, k) for k in (0, 1, 2, 0, 2, 1)]             # in order, around the epoch's end, out of order
    for k, g in zip((0, 1, 2, 0, 2, 1), got):
        assert_same_entries([g], [want[k]])
    assert res.upload_bytes > 0
    res.close()


def snapshot_one(res, k):
    e = res.load(k)
    return {name: (e[name].cpu().numpy() if isinstance(e[name], torch.Tensor) else e[name])
            for name in ("global_rows", "rows", "row0", "train", "test", "ref", "codes", "row_ids") if name in e}


def test_streamed_shuffled_entries_of_a_protein_table(prot_table):
    data = prot_table.shuffle(3)
    want = snapshot(build(data))
    assert want[0]["train"].shape[1] == 21 and [w["global_rows"] for w in want] == [250, 250, 100]
    file_order = snapshot(build(prot_table))
    assert not np.array_equal(file_order[0]["train"], want[0]["train"])      # (the rows did move)
    res = build(data, stream=True)
    assert res.streaming is True and res._by_range is True
    assert_same_entries(snapshot(res), want)


def test_alphabet_without_device_encoder_gathers_the_host_codes(monkeypatch):
    """An alphabet the device encoder does not know is encoded on the host (``_host_codes``), and the int8 codes are what is
    gathered.  Here the alphabet is dna under another name, so the entries must be those of the dna table (the two encoders
    agree: test_ingest_gpu.py)."""
    from bear_amd import core
    dna = ysd1_table()
    want = snapshot(build(dna.shuffle(3)))
    monkeypatch.setitem(core.alphabets_tf, "dna by another name", core.alphabets_tf["dna"])
    other = dataloader.CountDataset(dna.kmers, dna.counts, "dna by another name", dna.batch_size).shuffle(3)
    res = build(other, stream=True)
    assert res._fast_codes is False and res._host_codes.dtype == np.int8 and res._sources["codes"][0] is res._host_codes
    assert_same_entries(snapshot(res), want)


@pytest.mark.parametrize("stream", [False, True])
def test_rank_pieces_of_a_shuffled_table(stream, monkeypatch):
    """Rank 1 of 3 without a process group: its entries are the matching slices of the single-rank shuffled entries, whether its
    pieces stay resident (no whole column goes up: every piece is gathered by range) or are streamed."""
    data = ysd1_table().shuffle(3)
    kw = dict(drop_empty=None, kmer_order=False)        # (a piece sorted or compacted is no slice of the sorted, compacted batch)
    whole = snapshot(build(data, **kw))
    monkeypatch.setattr(dist, "world", lambda: (1, 3))
    monkeypatch.setattr(dist, "agree_max", lambda status, device: status)
    uploads = []
    monkeypatch.setattr(_train.ResidentBatches, "_upload_shuffled", lambda self: uploads.append(1) or {})
    pieces = data.rank_pieces(1, 3)
    res = build(data, stream=stream, **kw)
    assert res.streaming is stream and res._by_range is True
    got = snapshot(res)
    for g, w, (a, b), (g0, g1, _) in zip(got, whole, data.batch_bounds(), pieces):
        assert (g["global_rows"], g["rows"], g["row0"]) == (b - a, g1 - g0, g0) and 0 < g1 - g0 < b - a
        for name in ("train", "test", "ref", "codes"):
            assert g[name].dtype == w[name].dtype and np.array_equal(g[name], w[name][g0 - a:g1 - a]), name
        assert "row_ids" not in g
    assert uploads == []                                        # no rank sent a whole column up


# ------------------------------------------------------------------------------------------------ training and evaluation
def run_training(which, data, epochs=2):
    torch.manual_seed(11)
    ls, n = [], data.num_rows
    if which == "bear_ref + stop":
        out = bear_ref.train(data.repeat(epochs), n, epochs, 0, 2, "dna", 5, ar_funcs.make_ar_func_stop, {}, 0.01, "Adam", False, loss_save=ls)
    elif which == "bear_net + linear":
        out = bear_net.train(data.repeat(epochs), n, epochs, 0, "dna", 5, ar_funcs.make_ar_func_linear, {}, 0.01, "Adam", False, loss_save=ls)
    else:
        out = bear_net.train(data.repeat(epochs), n, epochs, 0, "prot", 4, ar_funcs.make_ar_func_linear, {}, 0.01, "Adam", False, loss_save=ls)
    return ls, np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in out[0]]), dict(_train.LAST_RUN), out


@pytest.mark.parametrize("which", ["bear_ref + stop", "bear_net + linear", "bear_net + linear, prot"])
def test_streamed_shuffled_training_equals_the_resident_shuffled_run(which, prot_table, monkeypatch):
    """Losses and parameters of data.shuffle(11).repeat(2), streamed, against the resident shuffled run; the
    held-out evaluation of bear_net likewise (accuracies exactly).  Comparison and tolerances: those of
    test_train_gpu.py::test_streamed_epochs_equal_resident_epochs."""
    data = (prot_table if which.endswith("prot") else ysd1_table()).shuffle(11)
    resident = run_training(which, data)
    assert len(resident[0]) == 3 * 2 and resident[2]["streaming"] is False
    file_order = run_training(which, prot_table if which.endswith("prot") else ysd1_table())
    assert not np.allclose(file_order[0], resident[0], rtol=1e-6, atol=0)       # (the shuffled batches are other batches)
    monkeypatch.setenv("BEAR_AMD_STREAM", "1")
    streamed = run_training(which, data)
    assert streamed[2]["streaming"] is True and streamed[2]["graph"] is False
    assert np.allclose(streamed[0], resident[0], rtol=1e-11, atol=0)
    assert np.allclose(streamed[1], resident[1], rtol=1e-8, atol=1e-10)
    if which.startswith("bear_net"):
        alphabet = "prot" if which.endswith("prot") else "dna"
        ev = lambda: bear_net.evaluation(data, 0, 1, alphabet, torch.exp(streamed[3][1]).detach(), streamed[3][2], np.array([0.1, 1.0]))
        got = ev()
        assert _train.LAST_RUN["streaming"] is True
        monkeypatch.delenv("BEAR_AMD_STREAM")
        want = ev()
        assert _train.LAST_RUN["streaming"] is False
        for a, b in zip(got, want):
            assert np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=1e-11, atol=0)
        for k in (6, 7, 8):                  # accuracies: counts of exactly decided arg-maxes over the same rows
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]))


def test_a_shuffled_table_that_does_not_fit_is_streamed_by_itself(monkeypatch):
    """The epoch's 1365 rows do not fit the free memory, the window of three batches of 300 does: the run streams, with the
    warning, and its losses are the resident shuffled run's."""
    data = dataloader.dataloader(YSD1, "dna", 300, 3).shuffle(11)          # five batches
    resident = run_training("bear_ref + stop", data)
    need = lambda rows: _train.hbm_budget_check(data, 2, False, device(), rows=rows)
    free = (need(900) + need(1365)) // 2
    assert need(900) < free < need(1365)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (free, 288 << 30))
    with pytest.warns(UserWarning, match="streaming the epoch"):
        auto = run_training("bear_ref + stop", data)
    assert auto[2]["streaming"] is True and len(auto[0]) == 5 * 2
    assert np.allclose(auto[0], resident[0], rtol=1e-11, atol=0)
    assert np.allclose(auto[1], resident[1], rtol=1e-8, atol=1e-10)
