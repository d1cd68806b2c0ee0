"""Times the width-generic kernels of the protein alphabet (kernels_wide.h) on synthetic sparse 21-wide contexts:
bear_dm_prior_wide_f64 in BEAR mode without and with gradient rows, and bear_eval_wide_f64 (one h, the AR model, three van_reg
values, with a training column).  HIP events; the clocks are settled first by back-to-back launches (as bench.py does).

    python scripts/prot_time.py [--rows 1e7] [--reps 20]

Prints one JSON line per kernel: ms per launch, bytes moved per context (counts 84 B + prior rows 168 B, + 168 B of gradient rows;
the evaluation also reads the test and training rows) and the fraction of 8 TB/s those bytes are."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bear_amd import kernels  # noqa: E402

W = 21
PEAK = 8.0e12


def synth(n, dev, seed):
    """Sparse protein rows: ~3 of 21 cells hold a count (Poisson-like, a few large), 10 % of the contexts hold none."""
    g = torch.Generator(dev).manual_seed(seed)
    lam = torch.exp(torch.rand(n, 1, device=dev, generator=g) * 6.0)                       # 1 .. 400 per context
    c = torch.poisson(lam.expand(n, W).contiguous(), generator=g)
    c = torch.where(torch.rand(n, W, device=dev, generator=g) < 0.15, c, torch.zeros_like(c))
    c[torch.rand(n, device=dev, generator=g) < 0.1] = 0
    return c.to(torch.int32).contiguous()


def settle(fn, cap_s=1.0):
    """Back-to-back launches until eight in a row take the same time within 1 % (or cap_s): the card's clocks have ramped."""
    t0, last = time.perf_counter(), None
    while time.perf_counter() - t0 < cap_s:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(8):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if last is not None and abs(ms - last) <= 0.01 * last:
            return
        last = ms


def timed(fn, reps):
    settle(fn)
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    n = int(a.rows)
    dev = torch.device("cuda", 0)
    counts, test = synth(n, dev, 1), synth(n, dev, 2)
    prior = torch.softmax(torch.randn(n, W, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(3)), dim=1)
    h = torch.tensor([0.3], dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    grad = torch.empty_like(prior)
    nz = float((counts != 0).float().mean())
    runs = [
        ("dm_prior_wide", 4 * W + 8 * W, lambda: kernels.dm_prior_wide(counts, prior, h, out=out)),
        ("dm_prior_wide+grad", 4 * W + 16 * W, lambda: kernels.dm_prior_wide(counts, prior, h, out=out, want_grad=True)),
        ("eval_wide", 8 * W + 8 * W, lambda: kernels.evaluate_wide(test, prior, [1.0], [0.1, 1.0, 10.0], counts, noise_seed=1)),
    ]
    for name, b, fn in runs:
        ms = timed(fn, a.reps)
        rate = n * b / (ms * 1e-3)
        print(json.dumps({"kernel": name, "rows": n, "width": W, "nonzero_cells": round(nz, 4), "ms": round(ms, 4),
                          "bytes_per_context": b, "TB_s": round(rate / 1e12, 3), "frac_of_8TB_s": round(rate / PEAK, 3)}), flush=True)


if __name__ == "__main__":
    main()
