"""Times one ``classify.classify`` call over the G groups of a table (bear_score_groups_f64, kernels_groups.h) against what gave
the same marginals before it: a loop over G ``DeviceCounter``s, one ``get_bear_probs_seqs(..., get_marg=True,
marg_on_device=True)`` call each.

    python scripts/classify_time.py [--table-rows 1e6] [--groups 8] [--proteins 3000] [--out profiles/classify_time.jsonl]

The case: the 1e6-row lag-5 protein table of scripts/score_time.py with G = 8 count columns, 3000 random proteins of 300 residues,
3 vanilla models.  Both paths run in this process on the same table, after one untimed call each: best and worst of three calls,
wall time around a synchronise.  The loop's scores must be the one call's bit for bit.  The kernels' own times (HIP events around
``kernels.score_groups`` and around the G ``kernels.score_marg`` calls, sorts included, best of three) say where a difference
comes from.  One JSON line is printed and appended to ``--out``."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import classify, core, dataloader, get_var_probs, kernels  # noqa: E402
from marg_time import VANS, emit  # noqa: E402
from prot_time import W  # noqa: E402
from score_time import make_table, wall  # noqa: E402


def kernel_ms(module_fn_name, call):
    """Milliseconds, summed over one ``call()``, that ``kernels.<module_fn_name>`` takes on the arguments ``call`` hands it: HIP events,
    best of three replays."""
    seen = []
    fn = getattr(kernels, module_fn_name)

    def keep(*args, **kw):
        seen.append((args, kw))
        return fn(*args, **kw)
    setattr(kernels, module_fn_name, keep)
    try:
        call()
    finally:
        setattr(kernels, module_fn_name, fn)
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for args, kw in seen:
            fn(*args, **kw)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best, len(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table-rows", type=float, default=1e6)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--proteins", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "classify_time.jsonl"))
    a = ap.parse_args()
    lag, G = 5, a.groups
    rng = np.random.default_rng(0)
    letters = list(core.alphabets_en["prot"][:20])
    seqs = ["".join(rng.choice(letters, 300)) for _ in range(a.proteins)]
    kmers, one = make_table(int(a.table_rows), seqs[0], lag, 1)
    n = len(kmers)
    counts = np.empty((G, n, W), dtype=np.uint32)            # column 0: make_table's; the others drawn the same way
    counts[0] = one.counts[0]
    for g in range(1, G):
        lam = np.exp(rng.random((n, 1)) * 5)
        counts[g] = np.where(rng.random((n, W)) < 0.15, rng.poisson(np.broadcast_to(lam, (n, W))), 0)
    data = dataloader.CountDataset(one.kmers, counts, "prot", 100000)
    group_counter = classify.GroupCounter.from_dataset(data)
    counters = [get_var_probs.DeviceCounter.from_dataset(data, g) for g in range(G)]

    def one_call():
        return classify.classify(group_counter, seqs, vans=VANS).log_marg

    def loop():
        return np.stack([get_var_probs.get_bear_probs_seqs(None, seqs, 0, vans=VANS, get_marg=True, lag=lag, alphabet_name="prot",
                                                           counter=c, marg_on_device=True) for c in counters], 1)
    got, call_best, call_worst = wall(one_call)
    want, loop_best, loop_worst = wall(loop)
    assert got.shape == want.shape == (len(seqs), G, 3) and got.tobytes() == want.tobytes()
    groups_ms, n_calls = kernel_ms("score_groups", one_call)
    marg_ms, n_marg = kernel_ms("score_marg", loop)
    assert n_marg == G
    emit({"call": "classify", "alphabet": "prot", "lag": lag, "table_rows": n, "groups": G, "sequences": len(seqs), "seq_len": 300,
          "models": 3, "one_call_s": [round(call_best, 4), round(call_worst, 4)], "loop_s": [round(loop_best, 4), round(loop_worst, 4)],
          "one_call_over_loop": round(call_best / loop_best, 4), "pieces": n_calls, "score_groups_ms": round(groups_ms, 4),
          "score_marg_x_groups_ms": round(marg_ms, 4), "equal_bits": True}, a.out)


if __name__ == "__main__":
    main()
