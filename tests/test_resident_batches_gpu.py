"""GPU characterisation of ``_train.ResidentBatches`` on its own (the training tests reach it only through whole runs): what a
batch entry holds after upload, encoding, the drop of the rows without training counts and the k-mer order -- resident, streamed,
shuffled on the device, and on a 21-wide table -- against a NumPy reconstruction from the host table.  All comparisons exact."""
import numpy as np
import pytest
import torch

from bear_amd import _train, dataloader
from conftest import YSD1
from test_prot_cpu import make_prot_table, write_prot_tsv

pytestmark = pytest.mark.gpu

COLUMNS = {"train": 0, "ref": 2}
TENSORS = ("train", "ref", "codes", "row_ids")


def ysd1_table():
    data = dataloader.dataloader(YSD1, "dna", 300, 3)           # 1365 rows: five batches, the last one short (165 rows)
    data.counts[0, ::4] = 0
    return data


def build(data, **kw):
    return _train.ResidentBatches(data, COLUMNS, torch.device("cuda", torch.cuda.current_device()), want_codes=True, drop_empty="train",
                                  kmer_order=True, **kw)


def expected_batches(data, sort=True):
    """Per batch: the rows with a training count, [in stable lexicographic order of their int8 codes, unknown letters last]."""
    codes = data.codes()
    out = []
    for a, b in data.batch_bounds():
        kept = np.nonzero((data.counts[0, a:b] != 0).any(axis=1))[0]
        if sort:
            key = codes[a:b][kept].astype(np.int64)
            key[key < 0] = 127
            kept = kept[np.lexsort(key.T[::-1])]                 # (lexsort: last key most significant, stable)
        out.append({"global_rows": b - a, "row0": a, "rows": len(kept), "row_ids": kept.astype(np.int32),
                    "train": data.counts[0, a:b][kept], "ref": data.counts[2, a:b][kept], "codes": codes[a:b][kept]})
    return out


def host(e):
    out = {name: e[name].cpu().numpy() for name in TENSORS}
    out["train"], out["ref"] = out["train"].view(np.uint32), out["ref"].view(np.uint32)
    return out


def assert_entry(e, want):
    assert (e["global_rows"], e["row0"], e["rows"]) == (want["global_rows"], want["row0"], want["rows"])
    got = host(e)
    for name in TENSORS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name


@pytest.fixture(scope="module")
def ysd1_expected():
    data = ysd1_table()
    want = expected_batches(data)
    assert len(want) == 5 and want[-1]["global_rows"] == 165 and all(0 < w["rows"] < w["global_rows"] for w in want)
    return want


def test_resident_batches_hold_the_kept_rows_in_kmer_order(ysd1_expected):
    res = build(ysd1_table())
    assert res.streaming is False and res.width == 5 and res.loads == 0 and len(res.batches) == 5
    for k, want in enumerate(ysd1_expected):
        assert res.load(k) is res.batches[k]
        assert_entry(res.batches[k], want)
    assert res.upload_bytes > 0
    res.close()


def test_streamed_batches_equal_the_resident_ones(ysd1_expected):
    res = build(ysd1_table(), stream=True)
    assert res.streaming is True and _train.LAST_RUN["streaming"] is True
    assert [e["_loaded"] for e in res.batches] == [False] * 5
    assert [(e["global_rows"], e["row0"], e["uploaded_rows"]) for e in res.batches] == [(w["global_rows"], w["row0"], w["global_rows"])
                                                                                         for w in ysd1_expected]
    held = list(res.batches)
    for _ in range(2):
        for k, want in enumerate(ysd1_expected):
            e = res.load(k)
            assert e is held[k] and res.batches[k] is held[k]          # the batch's dict is one object for the whole run
            assert [b["_loaded"] for b in res.batches] == [i == k for i in range(5)]
            assert e["uploaded_rows"] == want["global_rows"]
            assert_entry(e, want)
    assert res.loads == 10
    res.close()


def test_shuffled_batches_keep_the_columns_aligned():
    data = ysd1_table()
    want = expected_batches(data, sort=False)
    rows = lambda parts: sorted(map(bytes, np.concatenate([np.concatenate([p["train"].view(np.uint8), p["ref"].view(np.uint8),
                                                                           p["codes"].view(np.uint8)], axis=1) for p in parts])))
    res = build(data.shuffle(3))
    assert res.streaming is False and [e["global_rows"] for e in res.batches] == [300, 300, 300, 300, 165]
    got = [host(e) for e in res.batches]
    assert sum(e["rows"] for e in res.batches) == sum(w["rows"] for w in want)
    assert rows(got) == rows(want)
    assert any(not np.array_equal(g["train"], w["train"]) for g, w in zip(got, want))     # (and the rows did move)
    res.close()


def test_wide_table_stays_in_table_order_without_plans(tmp_path):
    kmers, counts = make_prot_table(seed=4, n=64, num_ds=3)
    write_prot_tsv(tmp_path / "prot.tsv", kmers, counts)
    data = dataloader.dataloader(str(tmp_path / "prot.tsv"), "prot", 40, 3)                # two batches: 40 and 24 rows
    want = expected_batches(data, sort=False)
    assert any(w["rows"] < w["global_rows"] for w in want)
    res = build(data, prebuild=[("train", 5, None)])
    assert res.width == 21 and len(res.batches) == 2
    for e, w in zip(res.batches, want):
        assert e["plans"] == {}
        if w["rows"] == w["global_rows"]:                          # no row dropped, none moved: no row_ids
            assert "row_ids" not in e
            e = dict(e, row_ids=torch.arange(w["rows"], dtype=torch.int32))
        assert_entry(e, w)
        assert e["train"].shape[1] == 21
    res.close()
