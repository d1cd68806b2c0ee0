"""Times one get_bear_probs call through the host ``counter=`` path and through the device path (a DeviceCounter), and the
score_sum kernel alone.

    python scripts/score_time.py [--table-rows 1e6] [--wt-len 300] [--mc 41] [--out profiles/score_time.jsonl]

The case of DESIGN 4.7: a lag-5 protein table, a random wild type and all of its single substitutions, 3 vanilla models.  Both
paths run in this process on the same table with the same seed: best and worst of three calls, wall time around a synchronise,
after one untimed call each.  The kernel: HIP events around back-to-back launches, after settling launches, on the arguments the
device path hands it.  One JSON line is printed and appended to ``--out``; the scores of the two paths are compared first."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import core, dataloader, get_var_probs, kernels  # noqa: E402
from prot_time import W, settle  # noqa: E402


def make_table(n_rows, wt, lag, seed):
    """A lag-`lag` protein table of n_rows distinct contexts as a CountDataset: every context of the wild type and a random fifth
    of the contexts of its single substitutions, the rest random; sparse Poisson counts (scripts/prot_sample_time.py's table)."""
    rng = np.random.default_rng(seed)
    letters = np.array(list(core.alphabets_en["prot"][:20]))
    pad = "[" * lag + wt + "]"
    must = {pad[j:j + lag] for j in range(len(pad) - lag)}
    for pos in range(len(wt)):
        for b in letters:
            if rng.random() < 0.2:
                s = pad[:lag + pos] + b + pad[lag + pos + 1:]
                must.update(s[j:j + lag] for j in range(pos, min(pos + lag + 1, len(s) - lag)))
    ids = np.unique(rng.integers(0, 20 ** lag, size=int(n_rows * 1.2)))
    rng.shuffle(ids)
    digits = (ids[:, None] // 20 ** np.arange(lag - 1, -1, -1)[None, :]) % 20
    rand = ["".join(r) for r in letters[digits]]
    kmers = sorted(set(list(must) + rand[:max(0, n_rows - len(must))]))[:n_rows]
    n = len(kmers)
    lam = np.exp(rng.random((n, 1)) * 5)
    counts = np.where(rng.random((n, W)) < 0.15, rng.poisson(np.broadcast_to(lam, (n, W))), 0).astype(np.uint32)
    kmer_bytes = np.frombuffer("".join(kmers).encode(), dtype=np.uint8).reshape(n, lag).copy()
    return kmers, dataloader.CountDataset(kmer_bytes, counts[None], "prot", 100000)


def wall(fn, reps=3):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table-rows", type=float, default=1e6)
    ap.add_argument("--wt-len", type=int, default=300)
    ap.add_argument("--mc", type=int, default=41)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_time.jsonl"))
    a = ap.parse_args()
    lag, vans = 5, [0.1, 1.0, 10.0]
    rng = np.random.default_rng(0)
    letters = list(core.alphabets_en["prot"][:20])
    wt = "".join(rng.choice(letters, a.wt_len))
    vars_ = [wt[p] + str(p) + b for p in range(len(wt)) for b in letters if b != wt[p]]
    kmers, data = make_table(int(a.table_rows), wt, lag, 1)
    row = {k: i for i, k in enumerate(kmers)}

    def host_counter(q):          # the host look-up a user had: a dictionary over the table's k-mer strings
        q = np.asarray(q)
        out = np.zeros((q.size, W))
        for i, k in enumerate(q.reshape(-1).tolist()):
            j = row.get(k)
            if j is not None:
                out[i] = data.counts[0, j]
        return out.reshape(q.shape + (W,))
    t0 = time.perf_counter()
    dev_counter = get_var_probs.DeviceCounter.from_dataset(data, 0)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0

    def call(counter):
        return get_var_probs.get_bear_probs(None, wt, vars_, 0, mc_samples=a.mc, vans=vans, lag=lag, alphabet_name="prot", seed=2,
                                            counter=counter)
    host, host_best, host_worst = wall(lambda: call(host_counter))
    dev, dev_best, dev_worst = wall(lambda: call(dev_counter))
    assert host.shape == dev.shape == (len(vars_), 3, a.mc) and np.isfinite(dev).all()
    diff = float(np.abs(host - dev).max())
    assert diff < 1e-9, diff

    # the kernel alone, on the arguments the device path hands it
    seen = {}
    score_sum = kernels.score_sum

    def keep(*args):
        seen["args"] = args
        return score_sum(*args)
    kernels.score_sum = keep
    try:
        call(dev_counter)
    finally:
        kernels.score_sum = score_sum
    lp, rows, letters_t, seg = seen["args"]
    settle(lambda: score_sum(lp, rows, letters_t, seg))
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            score_sum(lp, rows, letters_t, seg)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / a.reps)
    n_t = int((letters_t != kernels.SCORE_SKIP).sum())
    values = lp.shape[2] * lp.shape[3]
    moved = n_t * (5 + 8 * values) + rows.numel() * 5 + seg.numel() * 8 + (seg.numel() - 1) * values * 8
    line = {"call": "get_bear_probs", "alphabet": "prot", "lag": lag, "table_rows": len(kmers), "wt_len": len(wt), "variants": len(vars_),
            "models": 3, "mc": a.mc, "kmers_sampled": int(lp.shape[0]), "transitions": n_t,
            "host_counter_path_s": [round(host_best, 4), round(host_worst, 4)], "device_path_s": [round(dev_best, 4), round(dev_worst, 4)],
            "device_counter_setup_s": round(setup_s, 4), "max_abs_diff": diff, "score_sum_ms": round(best, 4),
            "score_sum_bytes_per_transition": 5 + 8 * values, "score_sum_GB_s": round(moved / (best * 1e-3) / 1e9, 1)}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
