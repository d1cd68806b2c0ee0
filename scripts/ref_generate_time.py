"""Times assemble.generate_sequences under a bear_ref model (generate_whole_ref_kernel of kernels_generate.h) on random protein tables.

    python scripts/ref_generate_time.py [--sequences 1000] [--max-len 1000] [--table-rows 1e6] [--lag 5]
                                        [--cases bmm,ref_stop,ref_stop_stepwise] [--out profiles/ref_generate_time.jsonl]

The workload of ``scripts/generate_whole_time.py`` (``--table-rows`` distinct random lag-``--lag`` protein contexts with sparse
Poisson counts) and a second table of as many rows, drawn with another seed, as the reference column: about a third of the
contexts of one are in the other.  Three cases: a BMM (``generate_whole_kernel``, the figure to hold the others against), a
stop-net ``bear_ref`` model in one launch (the mixing inside the kernel), and the same model stepwise (one launch per step on the
one-hot rows).  The model carries bear_ref's initial tau and net weight and h = 0.5: what a step costs does not depend on their
values.  Each case is the best and worst of three calls after one untimed call, wall time around a synchronise; one JSON line per
case is printed and appended to ``--out``."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
import numpy as np  # noqa: E402

from bear_amd import assemble, get_var_probs  # noqa: E402
from generate_time import random_table, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--max-len", type=int, default=1000)
    ap.add_argument("--table-rows", type=float, default=1e6)
    ap.add_argument("--lag", type=int, default=5)
    ap.add_argument("--cases", default="bmm,ref_stop,ref_stop_stepwise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_generate_time.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    kmers, data = random_table("prot", a.lag, int(a.table_rows), 1)
    ref_kmers, ref_data = random_table("prot", a.lag, int(a.table_rows), 2)
    counter, setup_s = timed(lambda: get_var_probs.DeviceCounter.from_dataset(data, 0))
    ref_counter, ref_setup_s = timed(lambda: get_var_probs.DeviceCounter.from_dataset(ref_data, 0))
    shared = int(np.isin(counter.keys.cpu().numpy(), ref_counter.keys.cpu().numpy()).sum())
    model = get_var_probs.RefModel(a.lag, "prot", 0.5, 1 / 30, 0.01)
    ref = dict(ref_model=model, ref_counter=ref_counter)
    models = {"bmm": dict(van=0.5), "ref_stop": ref, "ref_stop_stepwise": dict(stepwise=True, **ref)}
    for name in a.cases.split(","):
        def call():
            return assemble.generate_sequences(counter, a.sequences, a.max_len, seed=3, **models[name])
        call()
        times = []
        for _ in range(3):
            (seqs, stopped), t = timed(call)
            times.append(t)
        lens = np.array([len(s) for s in seqs.reshape(-1)])
        line = {"call": "generate_sequences", "case": name, "alphabet": "prot", "lag": a.lag, "table_rows": len(kmers),
                "ref_table_rows": len(ref_kmers), "contexts_in_both": shared, "sequences": a.sequences, "max_len": a.max_len,
                "seconds": [round(min(times), 4), round(max(times), 4)], "device_counter_setup_s": round(setup_s, 4),
                "ref_counter_setup_s": round(ref_setup_s, 4), "stopped": int(stopped.sum()), "mean_length": round(float(lens.mean()), 1),
                "longest": int(lens.max()), "letters_per_s": round(int(lens.sum()) / min(times))}
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
