"""What the plan builders produce, as numbers: sizes, tile cuts, pairings, prefix levels and window tables of a few small tables,
held to the values recorded in tests/golden/plan_shapes.json (written by this file run as a script on the commit before the host
units were split into phases).  A phase of plan construction that is lost, reordered or handed the wrong size shows up here as
a number, not as a slow or subtly different step.

Every value is a function of the table alone: none depends on the card (the cut's chunking goes by the table's length, the
pairing and the levels by its contexts), so none had to be left out.

    python tests/test_plan_shape_gpu.py OUT.json      # records the values of the library next to this file's tree
"""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_shapes.json")
LAG, FILTER_WIDTH = 5, 3
TABLES = ("rows0", "rows1", "rows3", "rows4", "ysd1", "sparse", "dense")


def _plan_constant(name):
    src = open(os.path.join(ROOT, "bear_amd", "csrc", "plan_common.h")).read()
    return int(re.search(r"#define %s (\d+)\b" % name, src).group(1))


def _table(case):
    """(train, test, ref) uint32 [n, 5] of the table ``case``."""
    import util
    if case.startswith("rows"):
        return tuple(c[:int(case[4:])] for c in util.sparse_table(4, 11))
    if case == "ysd1":
        import bear_oracle as o
        counts = o.parse_counts_tsv(os.path.join(ROOT, "tests", "golden", "ysd1_lag_5_file_0_preshuf.tsv"), 3)[1]
        return tuple(np.ascontiguousarray(counts[:, g]).astype(np.uint32) for g in range(3))
    if case == "sparse":
        # a tile holds at most PLN_RMAX contexts: more than two tiles' worth gives at least three; the last group of four is ragged
        n = 2 * _plan_constant("PLN_RMAX") + 5 * _plan_constant("PLN_QUAD") + 3
        return util.sparse_table(n, 3)
    train, ref = util.dense_table(3001, 2)
    return train, util.dense_table(3001, 4)[0], ref


def _codes(n):
    """k-mer-sorted letter codes [n, LAG] (a few start symbols), so that prefixes repeat and neighbours share leading letters"""
    rng = np.random.default_rng(n + 17)
    codes = rng.integers(0, 4, size=(n, LAG)).astype(np.int8)
    codes[rng.random((n, LAG)) < 0.03] = 4
    return np.ascontiguousarray(codes[np.lexsort(codes.T[::-1])])


def _plan_numbers(plan):
    row0, rows, items, off = plan.tiles()
    total, bound = plan.count_total()
    return {"bytes": plan.nbytes, "tile_count": len(row0), "row0": row0.tolist(), "rows": rows.tolist(), "items": items.tolist(),
            "stream_offset": off.tolist(), "count_total": total, "count_bound": bound}


def built_plans(case):
    """The numbers of bear_plan_create (five and four columns), _create_ref and _create_auto for the table: what BEAR_PLAN_CUT may
    not change."""
    import torch
    from bear_amd import kernels
    dev = torch.device("cuda", 0)
    train, _, ref = (torch.from_numpy(c.view(np.int32)).to(dev) for c in _table(case))
    auto = kernels.Plan(train, 5, rows_if_dense=True)
    return {"plan5": _plan_numbers(kernels.Plan(train, 5)), "plan4": _plan_numbers(kernels.Plan(train, 4)),
            "plan_ref": _plan_numbers(kernels.Plan(train, 4, ref=ref)), "plan_auto": dict(_plan_numbers(auto), rowwise=auto.rowwise)}


def attached(case):
    """What the other families hang on a five-column plan of the table, and the evaluation plan of its test column.  Pairing and
    attaching a second time replace the first: the plan's size stays where the first call left it (asserted here, for the
    recording run as for the test)."""
    import torch
    from bear_amd import kernels
    dev = torch.device("cuda", 0)
    train, test, _ = (torch.from_numpy(c.view(np.int32)).to(dev) for c in _table(case))
    code = kernels.pack_kmers(torch.from_numpy(_codes(train.shape[0])).to(dev))
    index = kernels.linear_index(code, LAG)
    plan = kernels.Plan(train, 5)
    out = {}
    paired = plan.pair_contexts(index, LAG)
    out["pair"] = {"paired": paired, "info": list(plan.pair_info()), "bytes": plan.nbytes}
    assert plan.pair_contexts(index, LAG) == paired and plan.nbytes == out["pair"]["bytes"]
    n_levels = plan.attach_cnn_levels(code, LAG, FILTER_WIDTH)
    rows, letters = plan.cnn_level_rows(with_letters=True)
    out["cnn"] = {"n_levels": n_levels, "level_rows": rows, "level_letters": letters,
                  "windows": [list(w) for w in plan.cnn_window_rows()], "bytes": plan.nbytes}
    assert plan.attach_cnn_levels(code, LAG, FILTER_WIDTH) == n_levels and plan.nbytes == out["cnn"]["bytes"]
    out["eval_plan_bytes"] = kernels.EvalPlan(test, train).nbytes
    return out


def kmer_sort_rows():
    """Rows (distinct contexts) that bear_kmer_sort_create / _wide find in a seeded text, per alphabet and lag."""
    from bear_amd import summarize
    rng = np.random.default_rng(5)
    out = {}
    for alphabet, letters, lags in (("dna", "ACGTN", (1, 3, 13)), ("prot", "ARNDCEQGHILKMFPSTWYVX", (1, 2, 5))):
        p = np.r_[np.full(len(letters) - 1, 0.99 / (len(letters) - 1)), 0.01]
        seqs = ["".join(rng.choice(list(letters), size=rng.integers(1, 200), p=p)) for _ in range(40)]
        text, group = summarize.encode_sequences(seqs, rng.integers(0, 2, len(seqs)), alphabet=alphabet)
        for lag in lags:
            out["%s_lag%d" % (alphabet, lag)] = int(summarize.count_transitions(text, group, lag, 2, alphabet=alphabet)[0].shape[0])
    return out


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TABLES)
def test_plan_shapes_are_the_recorded_ones(case, monkeypatch):
    want = _golden()[case]
    got = built_plans(case)
    assert got == want["built"], case
    if case == "sparse":
        assert got["plan5"]["tile_count"] >= 3 and got["plan5"]["rows"][-1] % _plan_constant("PLN_QUAD")
    if case == "dense":      # the dense form: nothing but the histograms, from both builders
        assert got["plan_auto"]["rowwise"] and got["plan_auto"]["tile_count"] == 0
        assert got["plan_ref"]["tile_count"] == 0 and got["plan_ref"]["bytes"] == got["plan_auto"]["bytes"]
    assert attached(case) == want["attached"], case
    monkeypatch.setenv("BEAR_PLAN_CUT", "host")      # the sequential definition of the cut: the same numbers
    assert built_plans(case) == want["built"], case


@pytest.mark.gpu
def test_kmer_sort_rows_are_the_recorded_ones():
    assert kmer_sort_rows() == _golden()["kmer_sort_rows"]


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    shapes = {case: {"built": built_plans(case), "attached": attached(case)} for case in TABLES}
    shapes["kmer_sort_rows"] = kmer_sort_rows()
    with open(sys.argv[1], "w") as fh:
        json.dump(shapes, fh, indent=1)
        fh.write("\n")
