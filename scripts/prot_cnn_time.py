"""Times the convolutional AR function of the protein alphabet as rows (kernels_cnn_wide.h) against its torch formulation:

  * cnn_forward_wide and cnn_backward_wide on random protein contexts (1e6 and 1e7; lag / filter width 1/1, 4/1, 5/3, 12/8, 16/8);
  * the torch formulation of the same function on the same codes (ar_funcs.make_ar_func_cnn with the width-21 kernels switched off:
    F.embedding_bag over the [n P, fw] int64 window indices, two layer norms, two tensordots, a softmax, and its autograd
    backward) -- what every caller ran before -- in the same process;
  * one bear_net.train step of a 1e6-row lag-12 protein table (one batch) with the HIP rows and with that torch formulation.

HIP events; the clocks are settled first by back-to-back launches (scripts/prot_time.py).  A train step is the device time of the
step loop per step, without the run's set-up and its first quarter of steps (_train.LAST_RUN), best of two runs.

    python scripts/prot_cnn_time.py [--out profiles/prot_cnn_time.jsonl] [--rows 1e6,1e7] [--shapes 1/1,4/1,5/3,12/8,16/8] [--no-train]

Appends one JSON line per figure to --out (and prints it).  The backward kernel's rate is given on the padded matrix products
(kernels_cnn_wide.h): per context and position 2 * 4 * 256 flop for every 16 x 16 x 4 product of the d filters (16-row tiles of
fw * 21 rows, two column tiles), d weights1 (two row tiles) and d intercept0 | d scale0 (four column tiles) sums, a quarter of a
product per context each."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bear_amd import ar_funcs, bear_net, core, dataloader, kernels  # noqa: E402
from prot_linear_time import contexts, emit  # noqa: E402
from prot_time import synth, timed  # noqa: E402

W = 21
PEAK_FP64_TFLOPS = 78.6
CHECK_CHUNK = 200_000


def torch_ar_func(lag, fw, dev, seed):
    """make_ar_func_cnn(lag, 20) as it dispatches without the width-21 kernels: torch ops on integer codes."""
    supported = kernels.cnn_supported
    kernels.cnn_supported = lambda lag, alphabet_size, *rest: alphabet_size == 4 and supported(lag, alphabet_size, *rest)
    try:
        f, params = ar_funcs.make_ar_func_cnn(lag, 20, filter_width=fw, device=dev, generator=torch.Generator(dev).manual_seed(seed))
    finally:
        kernels.cnn_supported = supported
    assert not f.fused
    return f, params


def best_of(fn, reps, rounds=3):
    """`timed` without its settling launches (for calls of a second each, made right after settled ones)."""
    fn()
    best = float("inf")
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def padded_flop_per_context(lag, fw):
    products = 2 * ((fw * W + 15) // 16) + 2 + 4          # per context and position, each over K = 1 of its 4 contexts
    return (lag - fw + 1) * products * 2 * 16 * 16


def time_rows(out, n, lag, fw, dev, reps):
    codes, q = contexts(n, lag, dev, 1000 * lag + fw)
    f, params = torch_ar_func(lag, fw, dev, 7)
    flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
    prior, t1 = kernels.cnn_forward_wide(codes, flat, lag, fw)
    ms_f = timed(lambda: kernels.cnn_forward_wide(codes, flat, lag, fw, save=False), reps)
    ms_fs = timed(lambda: kernels.cnn_forward_wide(codes, flat, lag, fw), reps)
    ms_b = timed(lambda: kernels.cnn_backward_wide(codes, flat, lag, fw, t1, prior, q), reps)
    slow = n > 2_000_000
    t_reps = 2 if slow else max(reps // 4, 2)
    with torch.no_grad():
        ms_tf = best_of(lambda: f(codes), t_reps) if slow else timed(lambda: f(codes), t_reps)

    def fb():
        for p in params:
            p.grad = None
        f(codes).backward(q)
    ms_tfb = best_of(fb, t_reps) if slow else timed(fb, t_reps)
    # the two agree (the figures compare the same function).  The torch side in chunks of CHECK_CHUNK contexts: its embedding-bag
    # stops agreeing with the one-hot formulation (and with these kernels) somewhere above 5e6 windows in one call
    for p in params:
        p.grad = None
    err_f = 0.0
    for i in range(0, n, CHECK_CHUNK):
        rows = f(codes[i:i + CHECK_CHUNK])
        rows.backward(q[i:i + CHECK_CHUNK])             # the gradients add up over the chunks
        err_f = max(err_f, float((rows.detach() / prior[i:i + CHECK_CHUNK] - 1).abs().max()))
    want = torch.cat([p.grad.reshape(-1) for p in params])
    g_hip = kernels.cnn_backward_wide(codes, flat, lag, fw, t1, prior, q)
    err_g, k = 0.0, 0
    for p in params:
        m = p.numel()
        err_g = max(err_g, float((g_hip[k:k + m] - want[k:k + m]).abs().max() / want[k:k + m].abs().max()))
        k += m
    f.clear_cache()
    base = {"rows": n, "lag": lag, "filter_width": fw, "width": W}
    tflops = n * padded_flop_per_context(lag, fw) / ms_b / 1e9
    emit(out, dict(base, what="cnn_forward_wide", ms=round(ms_f, 4), ms_with_t1=round(ms_fs, 4)))
    emit(out, dict(base, what="cnn_backward_wide", ms=round(ms_b, 4), TFLOP_s_padded=round(tflops, 2),
                   of_fp64_peak=round(tflops / PEAK_FP64_TFLOPS, 3)))
    emit(out, dict(base, what="torch_forward", ms=round(ms_tf, 4)))
    emit(out, dict(base, what="torch_forward_backward", ms=round(ms_tfb, 4)))
    emit(out, dict(base, what="ratio_torch_over_hip_forward_backward", ratio=round(ms_tfb / (ms_fs + ms_b), 2),
                   ratio_forward=round(ms_tf / ms_f, 2), max_rel_diff_rows=err_f, max_diff_grad_of_largest_per_tensor=err_g))


def train_ms_per_step(data, n, lag, fw, make, steps):
    """Device time per step of the later three quarters of a run's steps (HIP events of the step loop, _train.LAST_RUN), best of
    two runs; a run too short for that figure falls back to the wall time of the whole call over its steps."""
    from bear_amd import _train

    def run(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bear_net.train(data.repeat(epochs), n, epochs, 0, "prot", lag, make, {"filter_width": fw}, 0.01, "Adam", False)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / epochs
        timed = _train.LAST_RUN.get("timed_steps", 0)
        return _train.LAST_RUN["timed_ms"] / timed if timed else wall
    run(2)
    return min(run(steps), run(steps))


def time_train(out, n, lag, fw, dev):
    g = torch.Generator(dev).manual_seed(5)
    letters = torch.tensor([ord(c) for c in core.alphabets_en["prot"][:20]], dtype=torch.uint8, device=dev)
    kmers = letters[torch.randint(0, 20, (n, lag), device=dev, generator=g)]
    data = dataloader.DeviceCountDataset(kmers, synth(n, dev, 1)[None].contiguous(), "prot", n)

    def torch_make(lag, alphabet_size, filter_width=8, **kw):
        return torch_ar_func(lag, filter_width, kw.get("device"), 7)
    ms_hip = train_ms_per_step(data, n, lag, fw, ar_funcs.make_ar_func_cnn, 80)
    ms_torch = train_ms_per_step(data, n, lag, fw, torch_make, 12)
    base = {"rows": n, "lag": lag, "filter_width": fw, "width": W, "batch": n}
    emit(out, dict(base, what="bear_net_train_step_hip_rows", ms=round(ms_hip, 4)))
    emit(out, dict(base, what="bear_net_train_step_torch_rows", ms=round(ms_torch, 4)))
    emit(out, dict(base, what="ratio_train_step_torch_over_hip", ratio=round(ms_torch / ms_hip, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1e6,1e7")
    ap.add_argument("--shapes", default="1/1,4/1,5/3,12/8,16/8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for n in [int(float(x)) for x in a.rows.split(",") if x]:
        for lag, fw in [tuple(int(v) for v in x.split("/")) for x in a.shapes.split(",")]:
            time_rows(a.out, n, lag, fw, dev, a.reps)
    if not a.no_train:
        time_train(a.out, 1_000_000, 12, 8, dev)


if __name__ == "__main__":
    main()
