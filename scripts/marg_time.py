"""Times one get_bear_probs_seqs(..., get_marg=True) call through the host ``counter=`` loop and through the device path
(``marg_on_device=True`` with a DeviceCounter), and ``kernels.score_marg`` alone.

    python scripts/marg_time.py [--table-rows 1e6] [--proteins 3000] [--genome-len 1e6] [--long-genome-len 1.2e7]
                                [--out profiles/marg_time.jsonl]

Two cases.  prot: the residues of ``--proteins`` random 300-letter proteins on the 1e6-row lag-5 protein table of
scripts/score_time.py, 3 vanilla models.  dna: ONE sequence of ``--genome-len`` random letters at lag 8 on the table counted from
that sequence and its reverse complement (the host loop builds a Python list of the sequence's k+1-mers, which sets how long a
sequence it can be asked to take); the device path alone also takes one of ``--long-genome-len`` letters.  Both paths run in this
process on the same table: best and worst of three calls, wall time around a synchronise, after one untimed call each.
``score_marg`` (the sort and the three kernels): HIP events, best of three, on the arguments the device path hands it.  One JSON
line per case is printed and appended to ``--out``; the scores of the two paths are compared first."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import core, get_var_probs, kernels  # noqa: E402
from prot_time import W  # noqa: E402
from score_time import make_table, wall  # noqa: E402

VANS = [0.1, 1.0, 10.0]


def score_marg_alone(call):
    """(milliseconds of one ``kernels.score_marg``, positions, distinct k-mers) on the arguments ``call`` hands it."""
    seen = {}
    score_marg = kernels.score_marg

    def keep(*args):
        seen["args"] = args
        return score_marg(*args)
    kernels.score_marg = keep
    try:
        call()
    finally:
        kernels.score_marg = score_marg
    args = seen["args"]
    score_marg(*args)
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        score_marg(*args)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best, int(args[0].numel()), int(args[3].shape[0])


def compare(host, dev):
    assert host.shape == dev.shape and np.isfinite(dev).all()
    rel = float((np.abs(host - dev) / np.maximum(np.abs(host), 1.0)).max())
    assert rel < 1e-9, rel
    return rel


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as fh:
        fh.write(text + "\n")


def prot_case(a):
    lag = 5
    rng = np.random.default_rng(0)
    letters = list(core.alphabets_en["prot"][:20])
    seqs = ["".join(rng.choice(letters, 300)) for _ in range(a.proteins)]
    kmers, data = make_table(int(a.table_rows), seqs[0], lag, 1)
    row = {k: i for i, k in enumerate(kmers)}

    def host_counter(q):          # the host look-up a user had: a dictionary over the table's k-mer strings
        q = np.asarray(q)
        out = np.zeros((q.size, W))
        for i, k in enumerate(q.reshape(-1).tolist()):
            j = row.get(k)
            if j is not None:
                out[i] = data.counts[0, j]
        return out.reshape(q.shape + (W,))
    dev_counter = get_var_probs.DeviceCounter.from_dataset(data, 0)

    def call(counter, **kw):
        return get_var_probs.get_bear_probs_seqs(None, seqs, 0, vans=VANS, get_marg=True, lag=lag, alphabet_name="prot",
                                                 counter=counter, **kw)
    host, host_best, host_worst = wall(lambda: call(host_counter))
    dev, dev_best, dev_worst = wall(lambda: call(dev_counter, marg_on_device=True))
    rel = compare(host, dev)
    ms, n_pos, n_kmers = score_marg_alone(lambda: call(dev_counter, marg_on_device=True))
    emit({"call": "get_bear_probs_seqs get_marg", "alphabet": "prot", "lag": lag, "table_rows": len(kmers), "sequences": len(seqs),
          "seq_len": 300, "models": 3, "positions": n_pos, "kmers": n_kmers,
          "host_counter_path_s": [round(host_best, 4), round(host_worst, 4)], "device_path_s": [round(dev_best, 4), round(dev_worst, 4)],
          "max_rel_diff": rel, "score_marg_ms": round(ms, 4)}, a.out)


def dna_case(a):
    lag = 8
    rng = np.random.default_rng(1)
    letters = np.array(list(core.alphabets_en["dna"][:4]))
    genome = "".join(letters[rng.integers(0, 4, int(a.genome_len))])
    host_counter = get_var_probs.make_sequence_counter([genome], lag, reverse=True)
    dev_counter = get_var_probs.DeviceCounter.from_sequences([genome], lag, reverse=True)

    def call(counter, seq=genome, **kw):
        return get_var_probs.get_bear_probs_seqs(None, [seq], 0, vans=VANS, get_marg=True, lag=lag, alphabet_name="dna",
                                                 counter=counter, **kw)
    host, host_best, host_worst = wall(lambda: call(host_counter))
    dev, dev_best, dev_worst = wall(lambda: call(dev_counter, marg_on_device=True))
    rel = compare(host, dev)
    ms, n_pos, n_kmers = score_marg_alone(lambda: call(dev_counter, marg_on_device=True))
    line = {"call": "get_bear_probs_seqs get_marg", "alphabet": "dna", "lag": lag, "table_rows": int(dev_counter.keys.numel()),
            "sequences": 1, "seq_len": len(genome), "models": 3, "positions": n_pos, "kmers": n_kmers,
            "host_counter_path_s": [round(host_best, 4), round(host_worst, 4)], "device_path_s": [round(dev_best, 4), round(dev_worst, 4)],
            "max_rel_diff": rel, "score_marg_ms": round(ms, 4)}
    if a.long_genome_len:
        long_genome = "".join(letters[rng.integers(0, 4, int(a.long_genome_len))])
        _, long_best, long_worst = wall(lambda: call(dev_counter, seq=long_genome, marg_on_device=True))
        long_ms, long_pos, _ = score_marg_alone(lambda: call(dev_counter, seq=long_genome, marg_on_device=True))
        line.update({"long_seq_len": len(long_genome), "long_device_path_s": [round(long_best, 4), round(long_worst, 4)],
                     "long_positions": long_pos, "long_score_marg_ms": round(long_ms, 4)})
    emit(line, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table-rows", type=float, default=1e6)
    ap.add_argument("--proteins", type=int, default=3000)
    ap.add_argument("--genome-len", type=float, default=1e6)
    ap.add_argument("--long-genome-len", type=float, default=1.2e7)
    ap.add_argument("--cases", default="prot,dna")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "marg_time.jsonl"))
    a = ap.parse_args()
    for case in a.cases.split(","):
        {"prot": prot_case, "dna": dna_case}[case](a)


if __name__ == "__main__":
    main()
