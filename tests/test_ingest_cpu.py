"""CPU tests of the ingestion add-ons: the binary cache of a parsed table and the shuffle
permutation (host evaluation through the C ABI against the oracle restatement)."""
import ctypes
import os
import shutil

import numpy as np

import bear_oracle as o
from conftest import YSD1


def test_binary_cache_roundtrip_and_staleness(tmp_path, ysd1):
    from bear_amd import _lib, dataloader
    src = tmp_path / "table.tsv"
    shutil.copy(YSD1, src)
    cdir = tmp_path / "cache"
    d0 = dataloader.dataloader(str(src), "dna", 500, 3, binary_cache=str(cdir))
    cpath = dataloader.cache_path_for(str(src), str(cdir))
    assert os.path.exists(cpath)
    kmers, counts = ysd1                                         # oracle parse of the same file
    assert np.array_equal(d0.counts, counts.transpose(1, 0, 2).astype(np.uint32))
    # second load: served from the cache (the text is not needed any more -> make it unparsable but same size/mtime)
    st = os.stat(src)
    raw = src.read_bytes()
    src.write_bytes(b"#" * len(raw))
    os.utime(src, ns=(st.st_atime_ns, st.st_mtime_ns))
    d1 = dataloader.dataloader(str(src), "dna", 500, 3, binary_cache=str(cdir))
    assert np.array_equal(d1.counts, d0.counts) and np.array_equal(d1.kmers, d0.kmers)
    assert [bytes(r).decode() for r in d1.kmers[:3]] == list(kmers[:3])
    # a rank reads only its shard
    L = _lib.lib()
    km = np.zeros((100, 5), dtype=np.uint8)
    cn = np.zeros((3, 100, 5), dtype=np.uint32)
    assert L.bear_cache_read(cpath.encode(), 200, 100, km.ctypes.data, cn.ctypes.data) == 0
    assert np.array_equal(cn, d0.counts[:, 200:300]) and np.array_equal(km, d0.kmers[200:300])
    assert L.bear_cache_read(cpath.encode(), 1300, 100, km.ctypes.data, cn.ctypes.data) == -1   # beyond the table
    # stale: source rewritten with different content -> cache ignored and rebuilt
    src.write_bytes(raw[: raw.index(b"\n", 2000) + 1])
    d2 = dataloader.dataloader(str(src), "dna", 500, 3, binary_cache=str(cdir))
    assert d2.num_rows < d0.num_rows and np.array_equal(d2.counts, d0.counts[:, :d2.num_rows])
    n = ctypes.c_uint64()
    assert L.bear_cache_info(cpath.encode(), ctypes.byref(n), None, None, None, None) == 0 and n.value == d2.num_rows
    # a corrupt cache is rejected, not trusted
    with open(cpath, "r+b") as fh:
        fh.write(b"XXXX")
    assert L.bear_cache_info(cpath.encode(), ctypes.byref(n), None, None, None, None) == -7
    d3 = dataloader.dataloader(str(src), "dna", 500, 3, binary_cache=str(cdir))
    assert np.array_equal(d3.counts, d2.counts)


def test_shuffle_permutation_is_a_bijection_and_matches_the_abi():
    from bear_amd import kernels
    for n in [1, 2, 3, 5, 16, 17, 1365, 4097, 100003]:
        p = o.shuffle_perm(n, 20211012)
        assert np.array_equal(np.sort(p), np.arange(n))
        for i in {0, n // 3, n - 1}:
            assert kernels.shuffle_source_row(i, n, 20211012) == p[i]
    # different seeds give different orders; fixed points are rare
    a, b = o.shuffle_perm(10000, 1), o.shuffle_perm(10000, 2)
    assert (a != b).mean() > 0.99 and (a == np.arange(10000)).mean() < 0.01


def test_threaded_parser_matches_single_thread(tmp_path):
    """A table above the 1 MiB threshold is cut at line boundaries and parsed by several threads: same result as one
    thread, including blank lines and an error in the middle of the file."""
    from bear_amd import _lib, dataloader
    rng = np.random.default_rng(1)
    n, lag = 60000, 7
    letters = np.frombuffer(b"ACGT[", dtype=np.uint8)
    kmers = letters[rng.integers(0, 5, size=(n, lag))]
    counts = rng.integers(0, 5, size=(2, n, 5)).astype(np.uint32)
    counts[0, ::97, 0] = 4000000000
    path = tmp_path / "big.tsv"
    L = _lib.lib()
    assert L.bear_write_counts_tsv(str(path).encode(), kmers.ctypes.data, counts.ctypes.data, n, lag, 2, 0, 1, 0) == 0
    text = path.read_bytes()
    assert len(text) > (1 << 20)
    lines = text.split(b"\n")
    lines.insert(20000, b"")                       # blank lines are skipped (dataloader.py: CsvDataset ignores them too)
    lines.insert(45000, b"   ")
    path.write_bytes(b"\n".join(lines))
    results = []
    for threads in ("1", "8", "3"):
        os.environ["BEAR_PARSE_THREADS"] = threads
        d = dataloader.dataloader(str(path), "dna", 1000, 2)
        results.append(d)
        assert d.num_rows == n and np.array_equal(d.counts, counts) and np.array_equal(d.kmers, kmers)
    # a malformed row in the middle fails loudly whichever thread meets it
    bad = lines[:]
    bad[30000] = bad[30000].replace(b"[[", b"[[x")
    path.write_bytes(b"\n".join(bad))
    import pytest
    for threads in ("1", "8"):
        os.environ["BEAR_PARSE_THREADS"] = threads
        with pytest.raises(_lib.BearError):
            dataloader.dataloader(str(path), "dna", 1000, 2)
    os.environ.pop("BEAR_PARSE_THREADS")


def test_parser_fuzz_against_oracle(tmp_path):
    """Seeded random tables in the summarize.py row format, with the separators the reference's json.loads accepts
    (spaces after commas): the C++ reader and the oracle's parser agree on every one."""
    from bear_amd import dataloader
    rng = np.random.default_rng(11)
    for trial in range(20):
        n, lag, num_ds = int(rng.integers(1, 40)), int(rng.integers(1, 9)), int(rng.integers(1, 4))
        kmers = ["".join(rng.choice(list("ACGT["), size=lag)) for _ in range(n)]
        counts = rng.integers(0, 10 ** rng.integers(1, 10), size=(n, num_ds, 5))
        sep = ", " if trial % 2 else ","
        path = tmp_path / f"t{trial}.tsv"
        with open(path, "w") as fh:
            for k, rows in zip(kmers, counts):
                fh.write(k + "\t[[" + "],[".join(sep.join(str(int(v)) for v in g) for g in rows) + "]]\n")
                if trial % 5 == 0:
                    fh.write("\n")
        want_k, want_c = o.parse_counts_tsv(str(path), num_ds)
        d = dataloader.dataloader(str(path), "dna", 7, num_ds)
        assert [bytes(r).decode() for r in d.kmers] == list(want_k)
        assert np.array_equal(d.counts.transpose(1, 0, 2), want_c.astype(np.uint32))
        batches = list(d)
        assert sum(len(b[0]) for b in batches) == n and batches[0][1].shape[1:] == (num_ds, 5)


_BIG = {}


def _big_table():
    """The table of test_threaded_parser_matches_single_thread (60 000 rows, lag 7, 2 columns: 2.04 MB of text), generated once."""
    if not _BIG:
        rng = np.random.default_rng(1)
        n, lag = 60000, 7
        letters = np.frombuffer(b"ACGT[", dtype=np.uint8)
        kmers = letters[rng.integers(0, 5, size=(n, lag))]
        counts = rng.integers(0, 5, size=(2, n, 5)).astype(np.uint32)
        counts[0, ::97, 0] = 4000000000
        _BIG.update(kmers=kmers, counts=counts, text=_format_table(kmers, counts))
        assert len(_BIG["text"]) > (1 << 20)
    return _BIG["kmers"], _BIG["counts"], _BIG["text"]


def _format_table(kmers, counts):
    """`kmer \\t [[...],[...]] \\n` per row, formatted by Python from the arrays: no part of the library is in it."""
    n, lag = kmers.shape
    keys = kmers.tobytes().decode()
    fmt = "%s\t[" + ",".join(["[" + ",".join(["%d"] * counts.shape[2]) + "]"] * counts.shape[0]) + "]\n"
    rows = counts.transpose(1, 0, 2).reshape(n, -1).tolist()
    return "".join(fmt % (keys[i * lag:(i + 1) * lag], *r) for i, r in enumerate(rows)).encode()


def test_sharded_reader_above_the_thread_threshold(tmp_path, monkeypatch):
    """The sharded reader on several chunks (keep_shard and the shard_map::below offset of every chunk), behind a header line:
    every rank gets the generated rows at the indices dist.shard_rows gives per batch, the ranks cover the table once, and
    the file's row count comes back -- for one thread and for thread counts that do and do not divide the text evenly."""
    from bear_amd import _lib, dist
    kmers, counts, text = _big_table()
    n, lag = kmers.shape
    batch, world = 1000, 3
    path = tmp_path / "big.tsv"
    path.write_bytes(b"kmer\tcounts\n" + text)
    L = _lib.lib()
    for threads in ("1", "8", "3"):
        monkeypatch.setenv("BEAR_PARSE_THREADS", threads)
        seen = np.zeros(n, dtype=int)
        for r in range(world):
            idx = np.concatenate([a + np.arange(*dist.shard_rows(min(batch, n - a), r, world)) for a in range(0, n, batch)])
            km = np.full((len(idx), lag), 0xEE, dtype=np.uint8)
            cn = np.full((2, len(idx), 5), 0xEEEEEEEE, dtype=np.uint32)
            n_local, n_file = ctypes.c_uint64(), ctypes.c_uint64()
            st = L.bear_parse_counts_tsv_shard(str(path).encode(), 2, lag, 1, 0, n, batch, r, world, len(idx), km.ctypes.data,
                                               cn.ctypes.data, ctypes.byref(n_local), ctypes.byref(n_file))
            assert (st, n_local.value, n_file.value) == (0, len(idx), n), (threads, r)
            assert np.array_equal(km, kmers[idx]) and np.array_equal(cn, counts[:, idx]), (threads, r)
            seen[idx] += 1
        assert np.all(seen == 1), threads


def test_plain_reader_clips_at_max_rows(tmp_path, monkeypatch):
    """max_rows below the file's rows: status 0, max_rows rows, and nothing written behind them -- neither in the k-mer buffer
    nor behind counts[num_ds, max_rows, 5] -- whether one thread stops reading there or several threads clip their chunks."""
    from bear_amd import _lib
    kmers, counts, text = _big_table()
    n, lag = kmers.shape
    max_rows = 41234
    path = tmp_path / "big.tsv"
    path.write_bytes(text)
    L = _lib.lib()
    for threads in ("1", "8"):
        monkeypatch.setenv("BEAR_PARSE_THREADS", threads)
        km = np.full((n, lag), 0xEE, dtype=np.uint8)
        flat = np.full(2 * max_rows * 5 + 4096, 0xEEEEEEEE, dtype=np.uint32)
        cn, canary = flat[:2 * max_rows * 5].reshape(2, max_rows, 5), flat[2 * max_rows * 5:]
        got = ctypes.c_uint64()
        st = L.bear_parse_counts_tsv(str(path).encode(), 2, lag, max_rows, km.ctypes.data, cn.ctypes.data, ctypes.byref(got))
        assert (st, got.value) == (0, max_rows), threads
        assert np.array_equal(km[:max_rows], kmers[:max_rows]) and np.array_equal(cn, counts[:, :max_rows]), threads
        assert np.all(km[max_rows:] == 0xEE) and np.all(canary == 0xEEEEEEEE), threads


def test_writer_bytes_do_not_depend_on_threads(tmp_path, monkeypatch):
    """3 * 65536 + 17 rows give the writer up to four ranges of 64 Ki rows: with BEAR_PARSE_THREADS 1, 3 and 8 (one, three and
    four writer threads) the file is the text Python formats from the arrays, and a table written as four appended calls of
    every fourth row reads back as those rows."""
    from bear_amd import _lib
    rng = np.random.default_rng(5)
    n, lag = 3 * 65536 + 17, 6
    letters = np.frombuffer(b"ACGT[", dtype=np.uint8)
    kmers = letters[rng.integers(0, 5, size=(n, lag))]
    counts = (10 ** rng.integers(0, 10, size=(2, n, 5)) * rng.integers(0, 5, size=(2, n, 5))).clip(0, 2 ** 32 - 1).astype(np.uint32)
    want = _format_table(kmers, counts)
    order = np.concatenate([np.arange(j, n, 4) for j in range(4)])
    L = _lib.lib()
    whole, parts = tmp_path / "whole.tsv", tmp_path / "parts.tsv"
    for threads in ("1", "3", "8"):
        monkeypatch.setenv("BEAR_PARSE_THREADS", threads)
        assert L.bear_write_counts_tsv(str(whole).encode(), kmers.ctypes.data, counts.ctypes.data, n, lag, 2, 0, 1, 0) == 0
        assert whole.read_bytes() == want, threads
        for j in range(4):
            assert L.bear_write_counts_tsv(str(parts).encode(), kmers.ctypes.data, counts.ctypes.data, n, lag, 2, j, 4, int(j > 0)) == 0
        km = np.zeros((n, lag), dtype=np.uint8)
        cn = np.zeros((2, n, 5), dtype=np.uint32)
        got = ctypes.c_uint64()
        assert L.bear_parse_counts_tsv(str(parts).encode(), 2, lag, n, km.ctypes.data, cn.ctypes.data, ctypes.byref(got)) == 0
        assert got.value == n and np.array_equal(km, kmers[order]) and np.array_equal(cn, counts[:, order]), threads
