"""Times bear_ref's training step on the protein alphabet (kernels_refmix_wide.h) against the path it replaces:

  (a) the two kernels alone on synthetic sparse 21-wide contexts (prot_time.synth's density), 1e6 and 1e7 of them:
      dm_ref_wide (train + reference rows in: 168 B per context) and dm_refmix_wide_dev (+ net rows in, gradient rows out: 504 B),
      the bytes over the time as a share of 8 TB/s, next to dm_prior_wide with gradient rows (420 B) on the same counts -- the DM
      kernel of the former path, which holds the same fp64 items;
  (b) one bear_ref.train step (one batch = the table) with the stop net function and with the linear one at lag 5, on the new
      path and with BEAR_AMD_UNFUSED_MIX=1 -- the former path (the mixing as torch ops around dm_prior_wide), in the same process.
      A step is the difference of two runs of different length over the difference of their step counts (the set-up of a run
      cancels); the two paths alternate, three rounds: best and worst of each are reported, the spread between repeats of the same
      code being what "not slower" is read against.

HIP events for (a), after the clock-settling launches of scripts/prot_time.py.

    python scripts/prot_ref_time.py [--out profiles/prot_ref_time.jsonl] [--rows 1e6,1e7] [--no-train]

Appends one JSON line per figure to --out (and prints it)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bear_amd import ar_funcs, bear_ref, core, dataloader, kernels  # noqa: E402
from prot_time import PEAK, synth, timed  # noqa: E402

W = 21


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def time_kernels(out, n, dev, reps):
    train, ref = synth(n, dev, 1), synth(n, dev, 2)
    net = torch.softmax(torch.randn(n, W, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(3)), dim=1)
    h, tau, nw = (torch.tensor([v], dtype=torch.float64, device=dev) for v in (0.3, -1.2, -0.8))
    out4, out2 = torch.empty(4, dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.float64, device=dev)
    nz = float((train != 0).float().mean())
    live = float((train != 0).any(dim=1).float().mean())
    runs = [("dm_ref_wide", 8 * W, lambda: kernels.dm_ref_wide(train, ref, 0.3, -1.2, -0.8, out=out4)),
            ("dm_refmix_wide_dev", 24 * W, lambda: kernels.dm_refmix_wide_dev(train, net, ref, h, tau, nw, out=out4)),
            ("dm_prior_wide+grad", 20 * W, lambda: kernels.dm_prior_wide(train, net, h, out=out2, want_grad=True))]
    for name, b, fn in runs:
        ms = timed(fn, reps)
        rate = n * b / (ms * 1e-3)
        # fp64 items: one per non-zero training cell and one per context that holds any
        items = n * (nz * W + live)
        emit(out, {"what": name, "rows": n, "width": W, "nonzero_cells": round(nz, 4), "ms": round(ms, 4), "bytes_per_context": b,
                   "TB_s": round(rate / 1e12, 3), "frac_of_8TB_s": round(rate / PEAK, 3), "Gitems_s": round(items / ms / 1e6, 2)})


def train_s(data, n, lag, make, epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bear_ref.train(data.repeat(epochs), n, epochs, 0, 1, "prot", lag, make, {}, 0.01, "Adam", False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def time_train(out, n, lag, dev, short, long_):
    g = torch.Generator(dev).manual_seed(5)
    letters = torch.tensor([ord(c) for c in core.alphabets_en["prot"][:20]], dtype=torch.uint8, device=dev)
    kmers = letters[torch.randint(0, 20, (n, lag), device=dev, generator=g)]
    data = dataloader.DeviceCountDataset(kmers, torch.stack([synth(n, dev, 1), synth(n, dev, 2)]).contiguous(), "prot", n)
    for name, make in (("stop", ar_funcs.make_ar_func_stop), ("linear", ar_funcs.make_ar_func_linear)):
        ms = {"new": [], "unfused": []}

        def step_ms(path):
            if path == "unfused":
                os.environ["BEAR_AMD_UNFUSED_MIX"] = "1"
            try:
                a, b = train_s(data, n, lag, make, short), train_s(data, n, lag, make, long_)
            finally:
                os.environ.pop("BEAR_AMD_UNFUSED_MIX", None)
            return (b - a) / (long_ - short) * 1e3
        for path in ms:
            step_ms(path)                        # warm-up: allocator, algorithm choices
        for _ in range(3):
            for path in ms:
                ms[path].append(step_ms(path))
        base = {"rows": n, "lag": lag, "width": W, "batch": n, "net": name}
        for path, v in ms.items():
            emit(out, dict(base, what="bear_ref_train_step_" + path, ms=round(min(v), 4), ms_worst=round(max(v), 4)))
        emit(out, dict(base, what="ratio_unfused_over_new", ratio=round(min(ms["unfused"]) / min(ms["new"]), 2),
                       new_not_slower=bool(min(ms["new"]) <= max(ms["unfused"]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1e6,1e7")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for n in [int(float(x)) for x in a.rows.split(",")]:
        if not a.no_kernels:
            time_kernels(a.out, n, dev, a.reps)
        if not a.no_train:
            time_train(a.out, n, 5, dev, 6, 26)


if __name__ == "__main__":
    main()
