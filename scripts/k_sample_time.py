"""Times one k-sample call (bear_k_sample_f64, kernels_ksample.h) against what it replaces: the loop of G (G - 1) / 2 two-sample
calls (bear_two_sample_f64) over the pairs of G columns, one BEAR model each.  The tables of scripts/two_sample_time.py extended to
G = 2, 4, 8, 16 columns: 1e6 rows of a lag-5 protein table's shape (width 21, ~13 % of the cells non-zero) and 1e7 rows of width 5
(synthetic k=13 columns); each with every context seen in every sample ("all shared") and with a tenth of the contexts seen in
every sample and the rest in one sample only ("a tenth shared").

    python scripts/k_sample_time.py [--reps 20] [--rounds 5] [--prot-rows 1e6] [--dna-rows 1e7] [--groups 2 4 8 16]

Device time between events around back-to-back calls (`--reps`, fewer where the loop has many pairs), per call; the two variants
alternate over `--rounds` rounds after a warm-up round of each, and a figure is the median of its rounds with their smallest and
largest beside it.  One JSON line per table, sharing and G, appended to profiles/k_sample_time.jsonl.  At every timed size the two
are checked against each other: every group, pair and Bayes-factor sum within 2e-11 of a LOWER bound of its mass (the magnitudes of
the marginals it is formed from: the L1 mass of their terms is at least that), so the check asks more than the tests' bound."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import kernels  # noqa: E402
from two_sample_time import alternate  # noqa: E402

H = 0.7


def prot_table(n, G, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    cols = torch.empty((G, n, 21), dtype=torch.int32, device=dev)
    for k in range(G):
        lam = torch.rand((n, 1), device=dev, generator=g) * 20.0 + 0.5
        c = torch.poisson(lam.expand(n, 21), generator=g)
        cols[k] = (c * (torch.rand((n, 21), device=dev, generator=g) < 0.13)).to(torch.int32)
    f = torch.rand((n, 21), dtype=torch.float64, device=dev, generator=g) + 0.01
    return cols, f / f.sum(1, keepdim=True)


def dna_table(n, G, dev, seed):
    cols = torch.empty((G, n, 5), dtype=torch.int32, device=dev)
    for k in range(0, G, 2):
        t = kernels.synth_counts(seed + k, 0, n, dev, want=("train", "test"))
        cols[k], cols[k + 1] = t["train"], t["test"]
    return cols, kernels.synth_prior(seed, 0, n, dev)


def a_tenth_shared(cols, seed):
    """A tenth of the rows keep every sample, every other row one sample (drawn per row)."""
    G, n, _ = cols.shape
    g = torch.Generator(device=cols.device).manual_seed(seed)
    all_of_them = torch.rand(n, device=cols.device, generator=g) < 0.1
    only = torch.randint(0, G, (n,), device=cols.device, generator=g)
    keep = all_of_them.unsqueeze(0) | (only.unsqueeze(0) == torch.arange(G, device=cols.device).unsqueeze(1))
    return cols * keep.unsqueeze(2).to(cols.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prot-rows", type=float, default=1e6)
    ap.add_argument("--dna-rows", type=float, default=1e7)
    ap.add_argument("--groups", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k_sample_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    ok = True
    with open(args.out, "a") as fh:
        for name, make, n in (("prot lag 5, width 21", prot_table, int(args.prot_rows)), ("width 5", dna_table, int(args.dna_rows))):
            n -= n % 4                       # (columns of a multiple of four rows start on 16-byte boundaries: the table is used in place)
            full, f = make(n, max(args.groups), dev, 11)
            for sharing in ("all shared", "a tenth shared"):
                table = full if sharing == "all shared" else a_tenth_shared(full, 5)
                for G in args.groups:
                    cols = table[:G].contiguous()
                    pairs = [(g, g2) for g in range(G) for g2 in range(g + 1, G)]
                    reps = max(2, min(args.reps, 400 // len(pairs)))

                    def one_call():
                        return kernels.k_sample(cols, range(G), f, (H,), None)

                    def loop():
                        return [kernels.two_sample(cols[g], cols[g2], f, (H,), None)[0] for g, g2 in pairs]
                    t = alternate({"k_sample": one_call, "two_sample_loop": loop}, reps, args.rounds)
                    group, pair, _, _, _ = (None if x is None else x.cpu().numpy() for x in one_call())
                    want = np.stack([x.cpu().numpy()[0] for x in loop()])            # [P, 4] = {M_a, M_b, M_ab, B}
                    worst = 0.0
                    for p, (g, g2) in enumerate(pairs):
                        lower = [abs(want[p, 0]), abs(want[p, 1]), abs(want[p, 2]), abs(want[p, 0]) + abs(want[p, 1]) + abs(want[p, 2])]
                        got = [group[0, g], group[0, g2], pair[0, p, 0], pair[0, p, 1]]
                        worst = max(worst, max(abs(x - y) / max(m, 1e-300) for x, y, m in zip(got, want[p], lower)))
                    rec = {"table": name, "rows": n, "sharing": sharing, "groups": G, "pairs": len(pairs), "reps": reps, "rounds": args.rounds,
                           "ms_median_min_max": t, "loop_over_k_sample": round(t["two_sample_loop"][0] / t["k_sample"][0], 3),
                           "largest_difference_over_mass_lower_bound": float(worst), "agree_to_2e-11": bool(worst <= 2e-11),
                           "device": torch.cuda.get_device_name(0)}
                    ok = ok and rec["agree_to_2e-11"]
                    line = json.dumps(rec)
                    print(line, flush=True)
                    fh.write(line + "\n")
                    fh.flush()
            del full, f, table
    if not ok:
        sys.exit("k_sample and the two_sample loop differ by more than 2e-11 of the mass somewhere (see the lines above)")


if __name__ == "__main__":
    main()
