"""Times device k-mer counting (bear_count.hip: emit + radix sort + run-length reduce) at width 21 next to the 4-letter entry, on
synthetic texts of the same number of positions: sequences of 300 uniform letters, one group.  Per lag one handle is created and
reduced (bear_kmer_sort_create[_wide] + bear_kmer_sort_reduce) between two HIP events; the clocks are settled first by untimed
create + reduce rounds (as scripts/prot_time.py does), and the best of `--reps` timed rounds is kept.

    python scripts/prot_count_time.py [--positions 1e8] [--lags 3,6,12] [--reps 10]

Prints one JSON line per lag and appends it to profiles/prot_count_time.jsonl: ms for the protein and the DNA text, their ratio,
and the ratio of radix passes over 5 lag + 1 against 3 lag + 1 key bits (8 bits per pass) the sort-bound model predicts."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bear_amd import _lib  # noqa: E402

RADIX_BITS = 8      # key bits one pass of the library sort consumes (the model of the pass-count column, not a measured fact)


def synth_text(n_pos, seq_len, width, dev, seed):
    """start marker `width`, seq_len letters in [0, width - 1), stop `width - 1`, repeated."""
    reads = max(1, n_pos // (seq_len + 2))
    g = torch.Generator(dev).manual_seed(seed)
    body = torch.randint(0, width - 1, (reads, seq_len), dtype=torch.uint8, device=dev, generator=g)
    text = torch.cat([torch.full((reads, 1), width, dtype=torch.uint8, device=dev), body,
                      torch.full((reads, 1), width - 1, dtype=torch.uint8, device=dev)], 1).reshape(-1).contiguous()
    return text, torch.zeros_like(text)


def timed_count(L, text, grp, lag, width, wide, reps, settle_s=1.0):
    """-> (best ms of create + reduce, rows)."""
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    out = {}

    def one():
        h, n_rows = ctypes.c_void_p(), ctypes.c_uint64()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if wide:
            st = L.bear_kmer_sort_create_wide(text.data_ptr(), grp.data_ptr(), text.numel(), lag, width, ctypes.byref(h),
                                              ctypes.byref(n_rows), stream())
        else:
            st = L.bear_kmer_sort_create(text.data_ptr(), grp.data_ptr(), text.numel(), lag, ctypes.byref(h), ctypes.byref(n_rows), stream())
        _lib.check(st, "bear_kmer_sort_create")
        try:
            n = n_rows.value
            if out.get("n") != n:        # first round: the output slabs (their allocation falls into this, untimed, round)
                out.update(n=n, kmers=torch.empty((n, lag), dtype=torch.uint8, device=text.device),
                           counts=torch.empty((1, n, width), dtype=torch.int32, device=text.device))
            _lib.check(L.bear_kmer_sort_reduce(h, 1, out["kmers"].data_ptr(), None, out["counts"].data_ptr(), stream()), "bear_kmer_sort_reduce")
            e1.record()
            torch.cuda.synchronize()
        finally:
            L.bear_kmer_sort_destroy(h)
        return e0.elapsed_time(e1)
    t0 = time.perf_counter()
    one()
    while time.perf_counter() - t0 < settle_s:       # untimed settling rounds: the clocks ramp, the allocator's pools fill
        one()
    return min(one() for _ in range(reps)), out["n"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=float, default=1e8)
    ap.add_argument("--seq-len", type=int, default=300)
    ap.add_argument("--lags", default="3,6,12")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prot_count_time.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    n_pos = int(a.positions)
    prot = synth_text(n_pos, a.seq_len, 21, dev, 1)
    dna = synth_text(n_pos, a.seq_len, 5, dev, 2)
    passes = lambda bits: -(-bits // RADIX_BITS)      # noqa: E731
    with open(a.out, "a") as fh:
        for lag in (int(x) for x in a.lags.split(",")):
            ms_p, rows_p = timed_count(L, *prot, lag, 21, True, a.reps)
            ms_d, rows_d = timed_count(L, *dna, lag, 5, False, a.reps)
            rec = {"positions": prot[0].numel(), "seq_len": a.seq_len, "lag": lag, "prot_ms": round(ms_p, 3), "prot_rows": rows_p,
                   "dna_ms": round(ms_d, 3), "dna_rows": rows_d, "ratio": round(ms_p / ms_d, 3),
                   "key_bits": [5 * lag + 1, 3 * lag + 1], "pass_ratio": round(passes(5 * lag + 1) / passes(3 * lag + 1), 3),
                   "device": torch.cuda.get_device_name(0)}
            line = json.dumps(rec)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()


if __name__ == "__main__":
    main()
