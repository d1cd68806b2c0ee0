"""Times the linear AR function of the protein alphabet as rows (kernels_linrows_wide.h) against its torch formulation:

  * linear_forward_wide and linear_backward_wide on random protein contexts (1e6 and 1e7, lags 5 and 12);
  * the torch formulation of the same function on the same codes (ar_funcs.make_ar_func_linear with the kernels switched off:
    F.embedding_bag over an [n, lag] int64 index matrix + softmax, and its autograd backward) -- what every caller ran before;
  * one bear_net.train step of a 1e6-row lag-5 protein table (one batch) with the HIP rows and with that torch formulation.

HIP events; the clocks are settled first by back-to-back launches (scripts/prot_time.py).  A train step is the difference of two
runs of different length over the difference of their step counts (the set-up of a run cancels), best of three.

    python scripts/prot_linear_time.py [--out profiles/prot_linear_time.jsonl] [--rows 1e6,1e7] [--lags 5,12] [--no-train]

Appends one JSON line per figure to --out (and prints it)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bear_amd import ar_funcs, bear_net, core, dataloader, kernels  # noqa: E402
from prot_time import synth, timed  # noqa: E402

W = 21


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def contexts(n, lag, dev, seed):
    g = torch.Generator(dev).manual_seed(seed)
    codes = torch.randint(0, 20, (n, lag), dtype=torch.int8, device=dev, generator=g)
    codes[torch.rand(n, lag, device=dev, generator=g) < 0.03] = 20
    codes[torch.rand(n, lag, device=dev, generator=g) < 0.02] = -1
    q = torch.randn(n, W, dtype=torch.float64, device=dev, generator=g)
    q[torch.rand(n, device=dev, generator=g) < 0.3] = 0          # contexts without counts
    return codes.contiguous(), q


def torch_ar_func(lag, dev, seed):
    """make_ar_func_linear(lag, 20) as it dispatches without the width-21 kernels: torch ops on integer codes."""
    supported = kernels.linear_supported
    kernels.linear_supported = lambda lag, alphabet_size: alphabet_size == 4 and supported(lag, alphabet_size)
    try:
        f, (mat,) = ar_funcs.make_ar_func_linear(lag, 20, device=dev, generator=torch.Generator(dev).manual_seed(seed))
    finally:
        kernels.linear_supported = supported
    assert not f.fused
    return f, mat


def time_rows(out, n, lag, dev, reps):
    codes, q = contexts(n, lag, dev, 1000 * lag + 1)
    f, mat = torch_ar_func(lag, dev, 7)
    m = mat.detach().contiguous()
    prior = kernels.linear_forward_wide(codes, m, lag)
    ms_f = timed(lambda: kernels.linear_forward_wide(codes, m, lag), reps)
    ms_b = timed(lambda: kernels.linear_backward_wide(codes, lag, prior, q), reps)
    with torch.no_grad():
        ms_tf = timed(lambda: f(codes), max(reps // 4, 2))

    def fb():
        mat.grad = None
        f(codes).backward(q)
    ms_tfb = timed(fb, max(reps // 4, 2))
    # the two agree (the figures compare the same function)
    fb()
    g_hip = kernels.linear_backward_wide(codes, lag, prior, q)
    err_g = float((g_hip - mat.grad).abs().max() / mat.grad.abs().max())
    with torch.no_grad():
        err_f = float((f(codes) / prior - 1).abs().max())
    base = {"rows": n, "lag": lag, "width": W}
    emit(out, dict(base, what="linear_forward_wide", ms=round(ms_f, 4), TB_s=round(n * (lag + 8 * W) / ms_f / 1e9, 3)))
    emit(out, dict(base, what="linear_backward_wide", ms=round(ms_b, 4), TB_s=round(n * (lag + 16 * W) / ms_b / 1e9, 3),
                   GFLOP_s=round(n * 2 * 32 * ((lag * W + 15) // 16 * 16) / ms_b / 1e6, 1)))
    emit(out, dict(base, what="torch_forward", ms=round(ms_tf, 4)))
    emit(out, dict(base, what="torch_forward_backward", ms=round(ms_tfb, 4)))
    emit(out, dict(base, what="ratio_torch_over_hip_forward_backward", ratio=round(ms_tfb / (ms_f + ms_b), 2),
                   ratio_forward=round(ms_tf / ms_f, 2), max_rel_diff_rows=err_f, max_diff_grad_of_largest=err_g))


def train_ms_per_step(data, n, lag, make):
    def run(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bear_net.train(data.repeat(epochs), n, epochs, 0, "prot", lag, make, {}, 0.01, "Adam", False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    run(3)
    best = float("inf")
    for _ in range(3):
        a, b = run(10), run(60)
        best = min(best, (b - a) / 50 * 1e3)
    return best


def time_train(out, n, lag, dev):
    g = torch.Generator(dev).manual_seed(5)
    letters = torch.tensor([ord(c) for c in core.alphabets_en["prot"][:20]], dtype=torch.uint8, device=dev)
    kmers = letters[torch.randint(0, 20, (n, lag), device=dev, generator=g)]
    data = dataloader.DeviceCountDataset(kmers, synth(n, dev, 1)[None].contiguous(), "prot", n)

    def torch_make(lag, alphabet_size, **kw):
        f, mat = torch_ar_func(lag, kw.get("device"), 7)
        return f, [mat]
    ms_hip = train_ms_per_step(data, n, lag, ar_funcs.make_ar_func_linear)
    ms_torch = train_ms_per_step(data, n, lag, torch_make)
    base = {"rows": n, "lag": lag, "width": W, "batch": n}
    emit(out, dict(base, what="bear_net_train_step_hip_rows", ms=round(ms_hip, 4)))
    emit(out, dict(base, what="bear_net_train_step_torch_rows", ms=round(ms_torch, 4)))
    emit(out, dict(base, what="ratio_train_step_torch_over_hip", ratio=round(ms_torch / ms_hip, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1e6,1e7")
    ap.add_argument("--lags", default="5,12")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for n in [int(float(x)) for x in a.rows.split(",")]:
        for lag in [int(x) for x in a.lags.split(",")]:
            time_rows(a.out, n, lag, dev, a.reps)
    if not a.no_train:
        time_train(a.out, 1_000_000, 5, dev)


if __name__ == "__main__":
    main()
