"""Times bear_net's linear step at the protein alphabet's width as one launch (kernels_linear_wide.h) against the path it replaces:

  * the kernel alone (kernels.dm_linear_wide) next to the SUM of the three launches it replaces on the same inputs
    (linear_forward_wide, dm_prior_wide with gradient rows, linear_backward_wide), at 1e4 .. 1e7 contexts of prot_time.synth's
    density, lags 5 and 12;
  * one optimizer step of bear_net.train (one batch = the table, replayed from a HIP graph where the path captures one) on the new
    path and with BEAR_AMD_UNFUSED_LINEAR_WIDE=1, at the same sizes: the device time of the loop's later steps as
    run_device_steps measures it (HIP events on the launch stream, _train.LAST_RUN).

HIP events after the clock-settling launches (scripts/prot_time.py); the two paths alternate in one process, three rounds, best and
worst of each are reported.  The rule each comparison reports (scripts/prot_ref_time.py): the new path's best time lies within or
below the former path's best-to-worst spread (``new_not_slower``).

    python scripts/prot_linear_step_time.py [--out profiles/prot_linear_step_time.jsonl] [--rows 1e4,1e5,1e6,1e7] [--lags 5,12]

Appends one JSON line per figure to --out (and prints it)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bear_amd import _train, ar_funcs, bear_net, core, dataloader, kernels  # noqa: E402
from prot_time import settle, synth  # noqa: E402

W = 21


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def once(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def compare(out, base, what, paths, measure):
    """paths: {"new": ..., "former": ...}; measure(path) -> ms.  Alternating, three rounds."""
    ms = {p: [] for p in paths}
    for _ in range(3):
        for p in paths:
            ms[p].append(measure(p))
    for p, v in ms.items():
        emit(out, dict(base, what=f"{what}_{p}", ms=round(min(v), 4), ms_worst=round(max(v), 4)))
    emit(out, dict(base, what=f"{what}_ratio_former_over_new", ratio=round(min(ms["former"]) / min(ms["new"]), 2),
                   new_not_slower=bool(min(ms["new"]) <= max(ms["former"]))))


def contexts(n, lag, dev, seed):
    g = torch.Generator(dev).manual_seed(seed)
    codes = torch.randint(0, 20, (n, lag), dtype=torch.int8, device=dev, generator=g)
    codes[torch.rand(n, lag, device=dev, generator=g) < 0.03] = 20
    codes[torch.rand(n, lag, device=dev, generator=g) < 0.02] = -1
    return codes.contiguous()


def time_kernel(out, n, lag, dev):
    counts, codes = synth(n, dev, 1), contexts(n, lag, dev, 1000 * lag + 1)
    mat = (torch.randn(lag, W, W, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(7)) * 0.4).contiguous()
    h = torch.tensor([0.3], dtype=torch.float64, device=dev)
    out2 = torch.empty(2, dtype=torch.float64, device=dev)
    reps = max(4, min(200, int(2e7 // n)))

    def former():
        prior = kernels.linear_forward_wide(codes, mat, lag)
        _, q = kernels.dm_prior_wide(counts, prior, h, out=out2, want_grad=True)
        kernels.linear_backward_wide(codes, lag, prior, q)
    fns = {"new": lambda: kernels.dm_linear_wide(counts, codes, mat, 0.3, out=out2), "former": former}
    for fn in fns.values():
        settle(fn)
    base = {"rows": n, "lag": lag, "width": W, "nonzero_cells": round(float((counts != 0).float().mean()), 4)}
    compare(out, base, "kernel", fns, lambda p: once(fns[p], reps))


def time_train(out, n, lag, dev):
    g = torch.Generator(dev).manual_seed(5)
    letters = torch.tensor([ord(c) for c in core.alphabets_en["prot"][:20]], dtype=torch.uint8, device=dev)
    kmers = letters[torch.randint(0, 20, (n, lag), device=dev, generator=g)]
    data = dataloader.DeviceCountDataset(kmers, synth(n, dev, 1)[None].contiguous(), "prot", n)
    epochs = max(24, min(400, int(4e7 // n)))
    graph = {}

    def step_ms(path):
        if path == "former":
            os.environ["BEAR_AMD_UNFUSED_LINEAR_WIDE"] = "1"
        try:
            torch.manual_seed(1)
            bear_net.train(data.repeat(epochs), n, epochs, 0, "prot", lag, ar_funcs.make_ar_func_linear, {}, 0.01, "Adam", False)
        finally:
            os.environ.pop("BEAR_AMD_UNFUSED_LINEAR_WIDE", None)
        run = _train.LAST_RUN
        graph[path] = bool(run["graph"])
        return run["timed_ms"] / max(run["timed_steps"], 1)
    for path in ("new", "former"):
        step_ms(path)                            # warm-up: allocator, algorithm choices, the clocks
    base = {"rows": n, "lag": lag, "width": W, "batch": n, "steps": epochs}
    compare(out, base, "bear_net_train_step", {"new": None, "former": None}, step_ms)
    emit(out, dict(base, what="bear_net_train_step_graph", **graph))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1e4,1e5,1e6,1e7")
    ap.add_argument("--lags", default="5,12")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for n in [int(float(x)) for x in a.rows.split(",")]:
        for lag in [int(x) for x in a.lags.split(",")]:
            if not a.no_kernels:
                time_kernel(a.out, n, lag, dev)
            if not a.no_train:
                time_train(a.out, n, lag, dev)


if __name__ == "__main__":
    main()
