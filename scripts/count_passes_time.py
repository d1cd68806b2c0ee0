"""Times counting in passes over key ranges (bear_count.hip: bear_kmer_bin_hist + bear_kmer_sort_create_range) next to the single
pass (bear_kmer_sort_create), on one text: reads of 150 uniform letters in three groups, as tests/test_summarize_gpu.py's
test_full_size_count_conservation builds them.  Per lag: the histogram alone, the single pass, and the table in 1, 4 and 16 ranges
(summarize.count_transitions(..., on_device=True, max_pairs=m) with the smallest m that cuts the histogram into that many
ranges; the histogram is part of it).  Wall time around calls that end in a device synchronise, after untimed rounds of the
same call that settle the clocks and fill the allocator's pools; best and worst of `--reps` rounds.

    python scripts/count_passes_time.py [--positions 1e8] [--lags 5,13] [--ranges 1,4,16] [--reps 3]

Prints one JSON line per lag and appends it to profiles/count_passes_time.jsonl.  What the model expects: P ranges cost the
single pass plus (P + 1) scans of the text (the histogram and one compacting emit per range); `scan_ms` is the histogram's time,
`model_ms` = single + (P + 1) * scan_ms."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import _lib, summarize  # noqa: E402


def synth_text(n_pos, read_len, n_groups, dev, seed):
    reads = max(1, n_pos // (read_len + 2))
    g = torch.Generator(device=dev).manual_seed(seed)
    body = torch.randint(0, 4, (reads, read_len), dtype=torch.uint8, device=dev, generator=g)
    text = torch.cat([torch.full((reads, 1), 5, dtype=torch.uint8, device=dev), body,
                      torch.full((reads, 1), 4, dtype=torch.uint8, device=dev)], 1).reshape(-1).contiguous()
    grp = (torch.arange(reads, device=dev) % n_groups).to(torch.uint8).repeat_interleave(read_len + 2).contiguous()
    return text, grp


def timed(fn, reps, settle_s=1.0):
    """-> (best ms, worst ms) of `reps` rounds of fn(), which ends in a device synchronise, after untimed settling rounds."""
    t0 = time.perf_counter()
    fn()
    while time.perf_counter() - t0 < settle_s:
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(min(ms), 3), round(max(ms), 3)


def max_pairs_for(hist, n_ranges):
    """The smallest max_pairs that cuts `hist` into at most n_ranges ranges (bisection over cut_ranges)."""
    lo, hi = 1, int(hist.sum())
    while lo < hi:
        mid = (lo + hi) // 2
        if len(summarize.cut_ranges(hist, mid)) <= n_ranges:
            hi = mid
        else:
            lo = mid + 1
    return lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=float, default=1e8)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--lags", default="5,13")
    ap.add_argument("--ranges", default="1,4,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_passes_time.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    text, grp = synth_text(int(a.positions), a.read_len, a.groups, dev, 3)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with open(a.out, "a") as fh:
        for lag in (int(x) for x in a.lags.split(",")):
            n_bins = summarize.n_bins_of(lag)
            hist_dev = torch.empty(n_bins, dtype=torch.int64, device=dev)

            def hist_only():
                _lib.call("bear_kmer_bin_hist", text.data_ptr(), text.numel(), lag, 5, hist_dev.data_ptr(), n_bins, stream)
                torch.cuda.synchronize()

            def table(max_pairs):
                def run():
                    kmers, counts = summarize.count_transitions(text, grp, lag, a.groups, on_device=True, max_pairs=max_pairs)
                    torch.cuda.synchronize()
                    run.rows = kmers.shape[0]
                return run
            scan = timed(hist_only, a.reps)
            hist = hist_dev.cpu().numpy().view(np.uint64)
            single_fn = table(None)
            single = timed(single_fn, a.reps)
            rec = {"positions": text.numel(), "read_len": a.read_len, "groups": a.groups, "lag": lag, "pairs": int(hist.sum()),
                   "bins": n_bins, "scan_ms": list(scan), "single_ms": list(single), "rows": single_fn.rows, "passes": []}
            for p in (int(x) for x in a.ranges.split(",")):
                m = max_pairs_for(hist, p)
                fn = table(m)
                best, worst = timed(fn, a.reps)
                assert fn.rows == single_fn.rows
                rec["passes"].append({"ranges": len(summarize.cut_ranges(hist, m)), "max_pairs": m, "ms": [best, worst],
                                      "model_ms": round(single[0] + (p + 1) * scan[0], 3)})
            rec["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(rec)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()


if __name__ == "__main__":
    main()
