"""Times posterior sampling at the protein width: bear_logdir_sample_wide_f64 alone, and one get_bear_probs call split into its
parts.  HIP events for the kernel; the clocks are settled first by back-to-back launches (as bench.py does).

    python scripts/prot_sample_time.py [--kmers 1e5] [--table-rows 1e6] [--reps 10]

Prints one JSON line per measurement:
  - the sampler on sparse 21-wide k-mers with M = 4 models (1 h + 3 van) and mc = 41; the MAP table (AR + 1 h + 3 van); the same
    k-mers cut to 5 letters through bear_logdir_sample_f64;
  - one get_bear_probs call (vanilla models, mc = 41) on a synthetic protein table of lag 5: a 300-residue wild type and all of its
    single substitutions, split into the table scan, the sampler kernel, the device-to-host copy of its table, the rest of get_pdf,
    and the host scoring (_add_kmer_probs_vars)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import core, dataloader, get_var_probs, kernels  # noqa: E402
from prot_time import W, settle, synth  # noqa: E402


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


def kernel_runs(n, reps, dev):
    counts = synth(n, dev, 1)
    prior = torch.softmax(torch.randn(n, W, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(3)), dim=1)
    c5, p5 = counts[:, :5].contiguous(), (prior[:, :5] / prior[:, :5].sum(1, keepdim=True)).contiguous()
    h, vans, mc = [0.3], [0.1, 1.0, 10.0], 41
    runs = [
        ("logdir_sample_wide", W, 4, mc, lambda: kernels.logdir_sample_wide(counts, prior, h, vans, mc, seed=1)),
        ("logdir_sample_wide MAP", W, 5, 1, lambda: kernels.logdir_sample_wide(counts, prior, h, vans, 1, get_map=True, with_ar=True)),
        ("logdir_sample (W=5)", 5, 4, mc, lambda: kernels.logdir_sample(c5, p5, h, vans, mc, seed=1)),
        ("logdir_sample (W=5) MAP", 5, 5, 1, lambda: kernels.logdir_sample(c5, p5, h, vans, 1, get_map=True, with_ar=True)),
    ]
    for name, width, M, m, fn in runs:
        ms = timed(fn, reps)
        out_bytes = n * width * M * m * 8
        print(json.dumps({"kernel": name, "kmers": n, "width": width, "models": M, "mc": m, "ms": round(ms, 4),
                          "draws_per_ns": round(n * width * M * m / (ms * 1e6), 3) if m > 1 else None,
                          "out_MB": round(out_bytes / 1e6, 1), "out_TB_s": round(out_bytes / (ms * 1e-3) / 1e12, 3)}), flush=True)


def scan_table(path, n_rows, wt, lag, seed):
    """A lag-`lag` protein table of n_rows distinct contexts: every context of the wild type and a random fifth of the contexts of
    its single substitutions, the rest random; sparse Poisson counts."""
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
    counts = np.where(rng.random((n, W)) < 0.15, rng.poisson(np.broadcast_to(lam, (n, W))), 0)
    with open(path, "w") as fh:
        for k, row in zip(kmers, counts):
            fh.write(k + "\t[[" + ",".join(map(str, row)) + "]]\n")
    return n


def scoring_run(n_rows, dev):
    lag = 5
    rng = np.random.default_rng(0)
    wt = "".join(rng.choice(list(core.alphabets_en["prot"][:20]), 300))
    vars_ = [wt[p] + str(p) + b for p in range(len(wt)) for b in core.alphabets_en["prot"][:20] if b != wt[p]]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "protk5.tsv")
        n = scan_table(path, n_rows, wt, lag, 1)
        data = dataloader.dataloader(path, "prot", 100000, 1)
        t = {"kernel": 0.0, "d2h": 0.0, "get_pdf": 0.0, "host_scoring": 0.0, "kmers_sampled": 0}
        sample, pdf, add = kernels.logdir_sample_wide, get_var_probs.get_pdf, get_var_probs._add_kmer_probs_vars

        def sample_t(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = sample(*a, **k)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host = out.cpu()
            t["kernel"] += t1 - t0
            t["d2h"] += time.perf_counter() - t1
            t["kmers_sampled"] += out.shape[0]
            return host

        def timed_call(key, fn):
            def f(*a, **k):
                t0 = time.perf_counter()
                r = fn(*a, **k)
                t[key] += time.perf_counter() - t0
                return r
            return f
        kernels.logdir_sample_wide = sample_t
        get_var_probs.get_pdf = timed_call("get_pdf", pdf)
        get_var_probs._add_kmer_probs_vars = timed_call("host_scoring", add)
        try:
            get_var_probs.get_bear_probs(None, wt, vars_[:50], 0, mc_samples=41, lag=lag, alphabet_name="prot", data=data, seed=1)
            for key in ("kernel", "d2h", "get_pdf", "host_scoring", "kmers_sampled"):
                t[key] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scores = get_var_probs.get_bear_probs(None, wt, vars_, 0, mc_samples=41, lag=lag, alphabet_name="prot", data=data,
                                                  seed=2)
            total = time.perf_counter() - t0
        finally:
            kernels.logdir_sample_wide, get_var_probs.get_pdf, get_var_probs._add_kmer_probs_vars = sample, pdf, add
    assert np.isfinite(scores).all()
    rest = t["get_pdf"] - t["kernel"] - t["d2h"]
    print(json.dumps({"call": "get_bear_probs", "alphabet": "prot", "lag": lag, "table_rows": n, "wt_len": len(wt),
                      "variants": len(vars_), "models": 3, "mc": 41, "kmers_sampled": t["kmers_sampled"],
                      "total_s": round(total, 3), "table_scan_s": round(total - t["get_pdf"] - t["host_scoring"], 3),
                      "sampler_kernel_s": round(t["kernel"], 4), "d2h_copy_s": round(t["d2h"], 4),
                      "get_pdf_other_s": round(rest, 4), "host_scoring_s": round(t["host_scoring"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmers", type=float, default=1e5)
    ap.add_argument("--table-rows", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    kernel_runs(int(a.kmers), a.reps, dev)
    scoring_run(int(a.table_rows), dev)


if __name__ == "__main__":
    main()
