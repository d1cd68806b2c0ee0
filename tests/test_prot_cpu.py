"""The protein alphabet (20 letters + stop, rows of 21 counts) on the host: the text reader, the encoder, and the 5-wide paths
that refuse a 21-wide table.  No GPU needed."""
import json

import numpy as np
import pytest

from bear_amd import core, dataloader

PROT = "ARNDCEQGHILKMFPSTWYV"


def make_prot_table(seed=0, n=600, lag=4, num_ds=2):
    """A seeded sparse protein k-mer table: Poisson counts on a few cells per row, a handful of counts >= 1e5, some rows
    with no counts at all.  -> (k-mer strings, uint32 [num_ds, n, 21])."""
    rng = np.random.default_rng(seed)
    letters = np.array(list(PROT + "["))
    kmers = set()
    while len(kmers) < n:
        k = "".join(rng.choice(letters[:20], lag))
        pad = int(rng.integers(0, lag)) if rng.random() < 0.2 else 0       # start-padded contexts, as summarize writes them
        kmers.add("[" * pad + k[pad:])
    kmers = sorted(kmers)
    counts = np.zeros((num_ds, n, 21), dtype=np.uint32)
    for d in range(num_ds):
        mask = rng.random((n, 21)) < 0.15
        counts[d] = np.where(mask, rng.poisson(rng.uniform(0.5, 40.0, (n, 1)), (n, 21)), 0)
    big = rng.choice(n, min(6, n), replace=False)
    counts[0, big, rng.integers(0, 21, big.size)] = rng.integers(100_000, 3_000_000, big.size)
    counts[:, rng.choice(n, max(1, n // 24), replace=False)] = 0                            # rows without any count
    return kmers, counts


def write_prot_tsv(path, kmers, counts, header=False):
    with open(path, "w") as fh:
        if header:
            fh.write("kmer\tcounts\n")
        for i, k in enumerate(kmers):
            fh.write(k + "\t" + json.dumps(counts[:, i].tolist()).replace(" ", "") + "\n")


def parse_python(path, header):
    kmers, rows = [], []
    with open(path) as fh:
        if header:
            fh.readline()
        for line in fh:
            if line.strip():
                k, m = line.rstrip("\n").split("\t")
                kmers.append(k)
                rows.append(json.loads(m))
    return kmers, np.asarray(rows, dtype=np.uint64)        # [N, num_ds, 21]


@pytest.mark.parametrize("header", [False, True])
def test_prot_dataloader_matches_python_parse(tmp_path, header):
    kmers, counts = make_prot_table()
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts, header=header)
    data = dataloader.dataloader(str(path), "prot", 128, 2, header=header)
    want_k, want_c = parse_python(path, header)
    assert data.counts.shape == (2, len(kmers), 21) and data.width == 21 and data.lag == 4
    assert [bytes(r).decode() for r in data.kmers] == want_k
    np.testing.assert_array_equal(data.counts.transpose(1, 0, 2), want_c)
    np.testing.assert_array_equal(data.counts, counts)
    # the reference's batches: (kmers [B], counts [B, num_ds, 21])
    km, c = next(iter(data))
    assert c.shape == (128, 2, 21) and list(km[:3]) == [k.encode() for k in want_k[:3]]


def test_prot_sparse_dataloader_still_works(tmp_path):
    kmers, counts = make_prot_table(seed=3, n=50)
    path = tmp_path / "prot_sparse.tsv"
    with open(path, "w") as fh:
        fh.write("kmer;idx;vals\n")
        for i, k in enumerate(kmers):
            d, col = np.nonzero(counts[:, i])
            fh.write(f"{k};{json.dumps([[int(a), int(b)] for a, b in zip(d, col)])};"
                     f"{json.dumps([int(counts[a, i, b]) for a, b in zip(d, col)])}\n")
    data = dataloader.sparse_dataloader(str(path), "prot", 16, 2)
    np.testing.assert_array_equal(data.counts, counts)


def test_encode_kmers_prot_maps_every_letter():
    codes = core.encode_kmers([PROT[:10], PROT[10:], "[[[[[[[[[[", "ARNDXBZARN"], "prot")
    np.testing.assert_array_equal(codes[0], np.arange(10))
    np.testing.assert_array_equal(codes[1], np.arange(10, 20))
    np.testing.assert_array_equal(codes[2], np.full(10, 20))
    np.testing.assert_array_equal(codes[3], [0, 1, 2, 3, -1, -1, -1, 0, 1, 2])      # unknown letters: -1 (all-zero one-hot)


def test_bad_width_refused_by_the_reader(tmp_path):
    from bear_amd import _lib
    import ctypes
    kmers, counts = make_prot_table(n=10)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    km = np.zeros((10, 4), dtype=np.uint8)
    c = np.zeros((2, 10, 21), dtype=np.uint32)
    got = ctypes.c_uint64()
    L = _lib.lib()
    assert L.bear_parse_counts_tsv_wide(str(path).encode(), 2, 7, 4, 10, km.ctypes.data, c.ctypes.data, ctypes.byref(got)) == -1
    # 21-wide rows through the 5-wide width: a parse error, never 5-wide garbage
    c5 = np.zeros((2, 10, 5), dtype=np.uint32)
    assert L.bear_parse_counts_tsv_wide(str(path).encode(), 2, 5, 4, 10, km.ctypes.data, c5.ctypes.data, ctypes.byref(got)) != 0


def test_5_wide_paths_refuse_a_protein_table(tmp_path, monkeypatch):
    monkeypatch.delenv("BEAR_AMD_CACHE_DIR", raising=False)
    kmers, counts = make_prot_table(n=40)
    path = tmp_path / "prot.tsv"
    write_prot_tsv(path, kmers, counts)
    with pytest.raises(NotImplementedError, match="binary cache"):
        dataloader.dataloader(str(path), "prot", 16, 2, binary_cache=str(tmp_path / "cache"))
    with pytest.raises(NotImplementedError, match="binary cache"):
        monkeypatch.setenv("BEAR_AMD_CACHE_DIR", str(tmp_path / "cache"))
        dataloader.dataloader(str(path), "prot", 16, 2)
    monkeypatch.delenv("BEAR_AMD_CACHE_DIR")
    with pytest.raises(NotImplementedError, match="sharded reader"):
        dataloader.dataloader(str(path), "prot", 16, 2, shard=(0, 2))
    with pytest.raises(NotImplementedError, match="shard='kmer'"):
        dataloader.dataloader(str(path), "prot", 16, 2, shard="kmer")
    data = dataloader.dataloader(str(path), "prot", 16, 2)
    with pytest.raises(NotImplementedError, match="bmm_likelihood"):
        dataloader.bmm_likelihood(data, [1.0, 2.0])
    with pytest.raises(NotImplementedError, match="bmm_likelihood"):
        dataloader.bmm_likelihood(data.map(lambda k, c: c), [1.0])
    assert not list(tmp_path.glob("cache/*"))
