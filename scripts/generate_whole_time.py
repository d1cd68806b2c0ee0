"""Times assemble.generate_sequences (whole sequences from the start context to the stop, kernels_generate.h) on a random protein table.

    python scripts/generate_whole_time.py [--sequences 1000] [--max-len 1000] [--table-rows 1e6] [--lag 5]
                                          [--cases bmm,linear,linear_stepwise] [--out profiles/generate_whole_time.jsonl]

Three cases over the table of ``scripts/generate_time.py`` (``--table-rows`` distinct random lag-``--lag`` protein contexts with sparse
Poisson counts, the stop column among them): a BMM, a lag-``--lag`` linear BEAR model with the AR function inside the kernel (one
launch), and the same model stepwise (one AR call and one launch per step).  The linear model carries random weights of the size
training leaves: what a step costs does not depend on their values.  Each case is the best and worst of three calls after one
untimed call, wall time around a synchronise; the line also holds how long the sequences came out, since a sequence ends where it
draws the stop.  One JSON line per case is printed and appended to ``--out``."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import ar_funcs, assemble, get_var_probs  # noqa: E402
from generate_time import random_table, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--max-len", type=int, default=1000)
    ap.add_argument("--table-rows", type=float, default=1e6)
    ap.add_argument("--lag", type=int, default=5)
    ap.add_argument("--cases", default="bmm,linear,linear_stepwise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_whole_time.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    kmers, data = random_table("prot", a.lag, int(a.table_rows), 1)
    counter, setup_s = timed(lambda: get_var_probs.DeviceCounter.from_dataset(data, 0))
    ar_func, params = ar_funcs.make_ar_func_linear(a.lag, 20, device=counter.device, generator=torch.Generator(device=counter.device).manual_seed(1))
    with torch.no_grad():
        params[0].mul_(10.0)
    models = {"bmm": dict(van=0.5), "linear": dict(ar_func=ar_func, h=0.5), "linear_stepwise": dict(ar_func=ar_func, h=0.5, stepwise=True)}
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
                "sequences": a.sequences, "max_len": a.max_len, "seconds": [round(min(times), 4), round(max(times), 4)],
                "device_counter_setup_s": round(setup_s, 4), "stopped": int(stopped.sum()), "mean_length": round(float(lens.mean()), 1),
                "longest": int(lens.max()), "letters_per_s": round(int(lens.sum()) / min(times))}
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
