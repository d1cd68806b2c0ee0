"""Times ``moments=True`` -- the exact mean and variance of the scores -- against the sampled device path it replaces, for one
get_bear_probs and one get_bear_probs_seqs call.

    python scripts/moments_time.py [--tree DIR] [--label this] [--table-rows 1e6] [--wt-len 300] [--proteins 3000] [--mc 41]
                                   [--out profiles/moments_time.jsonl]

The scoring case of the README (scripts/score_time.py): a 1e6-row lag-5 protein table, a random 300-residue wild type and its 5700
single substitutions, 3 vanilla models; and the residues of ``--proteins`` random 300-letter proteins through get_bear_probs_seqs
(scripts/marg_time.py's).  Per call: the sampled device path at ``--mc`` samples (what a user reduces to a mean and a spread)
and, where the tree has the keyword, ``moments=True``; best and worst of three calls, wall time around a synchronise, after one
untimed call each; ``kernels.score_moments`` alone by HIP events.  The largest distance of the sample mean from the exact mean, in
standard errors sqrt(variance / mc), is recorded beside the times (tests/test_moments_gpu.py holds it to 6 at 4096 samples).

``--tree DIR`` imports ``bear_amd`` from another checkout (a build of the parent commit: the sampled path alone is timed there),
``--label`` names the run in the line; the project's habit is parent | this | parent, best of three each.  One JSON line per case
is printed and appended to ``--out``."""
import argparse
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--label", default="this")
    ap.add_argument("--table-rows", type=float, default=1e6)
    ap.add_argument("--wt-len", type=int, default=300)
    ap.add_argument("--proteins", type=int, default=3000)
    ap.add_argument("--mc", type=int, default=41)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "moments_time.jsonl"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "scripts")]
    import numpy as np
    import torch
    from bear_amd import core, get_var_probs, kernels
    from score_time import make_table, wall

    assert os.path.dirname(os.path.dirname(os.path.abspath(get_var_probs.__file__))) == tree
    has_moments = "moments" in inspect.signature(get_var_probs.get_bear_probs).parameters
    lag, vans = 5, [0.1, 1.0, 10.0]
    rng = np.random.default_rng(0)
    letters = list(core.alphabets_en["prot"][:20])
    wt = "".join(rng.choice(letters, a.wt_len))
    vars_ = [wt[p] + str(p) + b for p in range(len(wt)) for b in letters if b != wt[p]]
    seqs = ["".join(rng.choice(letters, 300)) for _ in range(a.proteins)]
    kmers, data = make_table(int(a.table_rows), wt, lag, 1)
    counter = get_var_probs.DeviceCounter.from_dataset(data, 0)
    common = dict(vans=vans, lag=lag, alphabet_name="prot", counter=counter)

    def kernel_alone(call):
        """Milliseconds of one ``kernels.score_moments`` (the sort, the prefix sum and the three kernels) on the arguments ``call``
        hands it, and its positions and distinct k-mers."""
        seen = {}
        score_moments = kernels.score_moments

        def keep(*args, **kw):
            seen["args"], seen["kw"] = args, kw
            return score_moments(*args, **kw)
        kernels.score_moments = keep
        try:
            call()
        finally:
            kernels.score_moments = score_moments
        score_moments(*seen["args"], **seen["kw"])
        best = float("inf")
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            score_moments(*seen["args"], **seen["kw"])
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best, int(seen["args"][0].numel()), int(seen["args"][3].shape[0])

    def case(name, sampled_call, moments_call, extra):
        sampled, s_best, s_worst = wall(sampled_call)
        line = dict({"call": name, "tree": a.label, "alphabet": "prot", "lag": lag, "table_rows": len(kmers), "models": 3, "mc": a.mc},
                    **extra)
        line["sampled_device_path_s"] = [round(s_best, 4), round(s_worst, 4)]
        if has_moments:
            exact, m_best, m_worst = wall(moments_call)
            assert exact.shape == sampled.shape[:2] + (2,) and np.isfinite(exact).all() and (exact[..., 1] >= 0).all()
            mean, var = exact[..., 0], exact[..., 1]
            z = np.abs(sampled.mean(-1) - mean) / np.sqrt(np.where(var > 0, var, 1.0) / a.mc)
            assert not np.abs(sampled.mean(-1) - mean)[var == 0].any()
            ms, n_pos, n_kmers = kernel_alone(moments_call)
            line.update({"moments_path_s": [round(m_best, 4), round(m_worst, 4)], "sampled_over_moments": round(s_best / m_best, 2),
                         "largest_mean_difference_in_standard_errors": round(float(z[var > 0].max()), 2), "positions": n_pos,
                         "kmers": n_kmers, "score_moments_ms": round(ms, 4)})
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")

    case("get_bear_probs",
         lambda: get_var_probs.get_bear_probs(None, wt, vars_, 0, mc_samples=a.mc, seed=2, **common),
         lambda: get_var_probs.get_bear_probs(None, wt, vars_, 0, moments=True, **common),
         {"wt_len": len(wt), "variants": len(vars_)})
    case("get_bear_probs_seqs",
         lambda: get_var_probs.get_bear_probs_seqs(None, seqs, 0, mc_samples=a.mc, seed=2, **common),
         lambda: get_var_probs.get_bear_probs_seqs(None, seqs, 0, moments=True, **common),
         {"sequences": len(seqs), "seq_len": 300})


if __name__ == "__main__":
    main()
