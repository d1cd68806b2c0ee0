"""Times the fused two-sample call (bear_two_sample_f64, kernels_twosample.h) against the composition that was available before
it: three bear_dm_prior_wide_f64 launches on `a`, `b` and a torch-made pooled column `a + b` (counts small enough not to wrap),
one BEAR model each.  Two tables: 1e6 rows of a lag-5 protein table's shape (width 21, ~13 % of the cells non-zero) and 1e7 rows of
width 5 (the synthetic k=13 table's train and test columns); each with every context shared by the two samples and with roughly a
tenth shared (the rest seen in one sample only: 45 % of the rows keep only `a`, 45 % only `b`).

    python scripts/two_sample_time.py [--reps 100] [--rounds 5] [--prot-rows 1e6] [--dna-rows 1e7]

Device time between events around `--reps` back-to-back calls, per call; the variants alternate over `--rounds` rounds after a
warm-up round of each, and a figure is the median of its rounds with their smallest and largest beside it.  One JSON line per
table and sharing, appended to profiles/two_sample_time.jsonl.  The composition's sums are not the fused call's bit for bit (its
h comes from exp(h_signed), and it forms the Bayes factor from three sums): the script checks only that the three marginals agree
to 1e-6 of the largest."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import kernels  # noqa: E402

H = 0.7


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants, reps, rounds):
    """{name: [median, smallest, largest] ms per call} of the variants {name: fn}, timed in turn in every round."""
    for fn in variants.values():
        event_ms(fn, max(1, reps // 4))
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(event_ms(fn, reps))
    return {name: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)] for name, v in ms.items()}


def prot_table(n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    cols = []
    for _ in range(2):
        lam = torch.rand((n, 1), device=dev, generator=g) * 20.0 + 0.5
        c = torch.poisson(lam.expand(n, 21), generator=g)
        keep = torch.rand((n, 21), device=dev, generator=g) < 0.13
        cols.append((c * keep).to(torch.int32))
    f = torch.rand((n, 21), dtype=torch.float64, device=dev, generator=g) + 0.01
    return cols[0], cols[1], f / f.sum(1, keepdim=True)


def dna_table(n, dev, seed):
    t = kernels.synth_counts(seed, 0, n, dev, want=("train", "test"))
    return t["train"], t["test"], kernels.synth_prior(seed, 0, n, dev)


def a_tenth_shared(a, b, seed):
    g = torch.Generator(device=a.device).manual_seed(seed)
    u = torch.rand(a.shape[0], device=a.device, generator=g)
    return a * (u < 0.55).unsqueeze(1).to(a.dtype), b * (u >= 0.45).unsqueeze(1).to(b.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prot-rows", type=float, default=1e6)
    ap.add_argument("--dna-rows", type=float, default=1e7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_sample_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    h_signed = torch.tensor([float(np.log(H))], dtype=torch.float64, device=dev)
    with open(args.out, "a") as fh:
        for name, make, n in (("prot lag 5, width 21", prot_table, int(args.prot_rows)), ("width 5", dna_table, int(args.dna_rows))):
            a0, b0, f = make(n, dev, 11)
            for sharing in ("all shared", "a tenth shared"):
                a, b = (a0, b0) if sharing == "all shared" else a_tenth_shared(a0, b0, 5)
                a, b = a.contiguous(), b.contiguous()
                both = float(((a.sum(1) > 0) & (b.sum(1) > 0)).double().mean())
                assert int(a.max()) + int(b.max()) < 2 ** 31                 # the pooled int32 column does not wrap
                outs = [torch.empty(2, dtype=torch.float64, device=dev) for _ in range(3)]

                def composed():
                    pooled = a + b
                    for c, o in zip((a, b, pooled), outs):
                        kernels.dm_prior_wide(c, f, h_signed, eps=0.0, out=o)

                def fused(hs=(H,), rows=False):
                    return kernels.two_sample(a, b, f, hs, None, want_rows=rows)
                rec = {"table": name, "rows": n, "sharing": sharing, "rows_with_both_samples": round(both, 4), "reps": args.reps,
                       "rounds": args.rounds, "ms_median_min_max": alternate(
                           {"fused_1_model": fused, "composed_1_model": composed, "fused_4_models": lambda: fused((0.05, H, 3.0, 20.0)),
                            "fused_1_model_with_row_terms": lambda: fused(rows=True)}, args.reps, args.rounds)}
                t = rec["ms_median_min_max"]
                rec["composed_over_fused"] = round(t["composed_1_model"][0] / t["fused_1_model"][0], 3)
                got = fused()[0].cpu().numpy()[0]
                want = np.array([o.cpu().numpy()[0] for o in outs])
                assert np.abs(got[:3] - want).max() <= 1e-6 * np.abs(want).max(), (got, want)
                rec["log_bf"] = float(got[3])
                rec["device"] = torch.cuda.get_device_name(0)
                line = json.dumps(rec)
                print(line, flush=True)
                fh.write(line + "\n")
                fh.flush()
            del a0, b0, f


if __name__ == "__main__":
    main()
