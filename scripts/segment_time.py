"""Times ``classify.segment`` (bear_score_emit_groups_f64 + bear_hmm_groups_f64, kernels_segment.h) against what a user could write
before it: the same recurrences as a torch log-space loop on the device, one step per position, batched over the sequences.

    python scripts/segment_time.py [--reads 1e5] [--long 5e6] [--loop-positions 2e5] [--out profiles/segment_time.jsonl]

Regime (a), many short sequences: ``--reads`` reads of 150 nt against a lag-8 dna table of 8 groups.  Regime (b), one long
sequence: one ``--long``-letter sequence against a lag-8 table of 4 groups; the torch loop is timed on the first
``--loop-positions`` positions only and reported PER POSITION next to the one call's time per position -- nothing is extrapolated
to the whole sequence.  van(1), switch probability 0.005.  Wall time around a synchronise, best and worst of three after one
untimed call; HIP events (best of three replays) for the two entries.  The loop's results must agree with the entry's within the
bounds of tests/test_segment_gpu.py: scalars and posteriors within 1e-11 of the mass, the path equal wherever the loop's two best
max-marginals lie more than 1e-6 apart.  One JSON line per regime is printed and appended to ``--out``."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import classify, kernels  # noqa: E402
from classify_time import kernel_ms  # noqa: E402
from marg_time import emit  # noqa: E402
from score_time import wall  # noqa: E402

LAG, SWITCH, VANS, RTOL, MIN_GAP = 8, 0.005, [1.0], 1e-11, 1e-6


def draw(rng, comp, n):
    return "".join(np.array(list("ACGT"))[rng.choice(4, n, p=comp)])


def make_counter(rng, G):
    """A lag-8 table of G groups, each counted on 200 sequences of 1000 letters of its own composition -> (counter, compositions)."""
    comps = rng.dirichlet(np.full(4, 3.0), size=G)
    return classify.GroupCounter.from_sequences([[draw(rng, comps[g], 1000) for _ in range(200)] for g in range(G)], LAG), comps


def torch_loop(e, lt, ls):
    """Both recurrences of include/bear_hip.h, one step per position: ``e`` [n, T, G] on the device -> (log_evidence [n], log_best [n],
    path [n, T], log_post [n, T, G], gap [n, T])."""
    n, T, G = e.shape
    alpha, delta = torch.empty_like(e), torch.empty_like(e)
    a = ls + e[:, 0]
    d = a.clone()
    alpha[:, 0], delta[:, 0] = a, d
    for t in range(1, T):
        a = e[:, t] + torch.logsumexp(a[:, :, None] + lt, 1)
        d = e[:, t] + (d[:, :, None] + lt).max(1).values
        alpha[:, t], delta[:, t] = a, d
    ev, best = torch.logsumexp(a, 1), d.max(1).values
    post, mm = torch.empty_like(e), torch.empty_like(e)
    b, h = torch.zeros_like(a), torch.zeros_like(a)
    post[:, T - 1], mm[:, T - 1] = a - ev[:, None], d
    for t in range(T - 2, -1, -1):
        b = torch.logsumexp(lt[None] + (e[:, t + 1] + b)[:, None, :], 2)
        h = (lt[None] + (e[:, t + 1] + h)[:, None, :]).max(2).values
        post[:, t], mm[:, t] = alpha[:, t] + b - ev[:, None], delta[:, t] + h
    top = mm.topk(2, dim=2).values
    return ev, best, mm.argmax(2), post, top[..., 0] - top[..., 1]


def agree(e, lt, ls, loop, entry):
    """The loop's results against the entry's on the same emissions [n, T, G] -> the largest error / mass."""
    n, T, G = e.shape
    mass = e.abs().max(2).values.sum(1) + (T - 1) * lt.abs().max() + ls.abs().max()
    ev, best, path, post, gap = loop
    ev2, best2, path2, post2 = entry
    worst = max(float(((ev - ev2).abs() / mass).max()), float(((best - best2).abs() / mass).max()),
                float(((post - post2.reshape(n, T, G)).abs().amax((1, 2)) / mass).max()))
    decided = gap > MIN_GAP
    assert worst <= RTOL, worst
    assert bool((path[decided] == path2.reshape(n, T).long()[decided]).all()) and float(decided.double().mean()) > 0.99
    return worst


def entry_ms(call):
    ms_emit, _ = kernel_ms("emit_groups", call)
    ms_hmm, pieces = kernel_ms("hmm_groups", call)
    return ms_emit, ms_hmm, pieces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=1e5)
    ap.add_argument("--long", type=float, default=5e6)
    ap.add_argument("--loop-positions", type=float, default=2e5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "segment_time.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")

    def chain(G):
        lt = np.full((G, G), np.log(SWITCH / (G - 1)))
        np.fill_diagonal(lt, np.log1p(-SWITCH))
        return torch.from_numpy(lt).to(dev), torch.full((G,), -np.log(G), dtype=torch.float64, device=dev)

    # ---- (a) many short sequences
    G, n_reads, length = 8, int(a.reads), 150
    counter, comps = make_counter(rng, G)
    reads = [draw(rng, comps[i % G], 75) + draw(rng, comps[(i + 1) % G], 75) for i in range(n_reads)]

    def one_call():
        return classify.segment(counter, reads, vans=VANS, switch=SWITCH)
    res, call_best, call_worst = wall(one_call)
    ms_emit, ms_hmm, pieces = entry_ms(one_call)
    T = length + 1
    e = torch.from_numpy(classify.position_log_probs(counter, reads, vans=VANS).log_prob[:, :, 0]).to(dev).reshape(n_reads, T, G)
    lt, ls = chain(G)
    loop, loop_best, loop_worst = wall(lambda: torch_loop(e, lt, ls))
    seg = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * T
    worst = agree(e, lt, ls, loop, kernels.hmm_groups(e.reshape(-1, G), seg, lt.cpu().numpy(), ls.cpu().numpy()))
    assert res.path.size == n_reads * T
    emit({"call": "segment", "regime": "a: many short sequences", "lag": LAG, "groups": G, "sequences": n_reads, "seq_len": length,
          "positions": n_reads * T, "one_call_s": [round(call_best, 4), round(call_worst, 4)], "pieces": pieces,
          "emit_groups_ms": round(ms_emit, 4), "hmm_groups_ms": round(ms_hmm, 4),
          "torch_loop_chain_only_s": [round(loop_best, 4), round(loop_worst, 4)],
          "torch_loop_over_hmm_groups": round(loop_best * 1e3 / ms_hmm, 2), "largest_error_over_mass": worst}, a.out)
    del e, loop, res

    # ---- (b) one long sequence
    G, n_long, n_loop = 4, int(a.long), int(a.loop_positions)
    counter, comps = make_counter(rng, G)
    block = 50000
    long_seq = "".join(draw(rng, comps[(i // block) % G], min(block, n_long - i)) for i in range(0, n_long, block))

    def one_long():
        return classify.segment(counter, [long_seq], vans=VANS, switch=SWITCH)
    res, call_best, call_worst = wall(one_long)
    ms_emit, ms_hmm, pieces = entry_ms(one_long)
    P = res.path.size
    truth = np.repeat(np.arange((n_long + block - 1) // block) % G, block)[:n_long]
    accuracy = float((res.path[:n_long] == truth).mean())
    head = long_seq[:n_loop - 1]                              # its transitions: the letters and the stop, n_loop in all
    e = torch.from_numpy(classify.position_log_probs(counter, [head], vans=VANS).log_prob[:, :, 0]).to(dev).reshape(1, n_loop, G)
    lt, ls = chain(G)
    loop, loop_best, loop_worst = wall(lambda: torch_loop(e, lt, ls))
    seg = torch.tensor([0, n_loop], dtype=torch.int64, device=dev)
    worst = agree(e, lt, ls, loop, kernels.hmm_groups(e.reshape(-1, G), seg, lt.cpu().numpy(), ls.cpu().numpy()))
    per_call, per_entries, per_loop = call_best / P * 1e9, (ms_emit + ms_hmm) * 1e6 / P, loop_best / n_loop * 1e9
    assert per_call < per_loop, (per_call, per_loop)          # the chunk cut buys what it is for
    emit({"call": "segment", "regime": "b: one long sequence", "lag": LAG, "groups": G, "positions": P, "pieces": pieces,
          "one_call_s": [round(call_best, 4), round(call_worst, 4)], "emit_groups_ms": round(ms_emit, 4), "hmm_groups_ms": round(ms_hmm, 4),
          "torch_loop_positions": n_loop, "torch_loop_chain_only_s": [round(loop_best, 4), round(loop_worst, 4)],
          "ns_per_position": {"one_call_wall": round(per_call, 2), "two_entries": round(per_entries, 3), "hmm_groups": round(ms_hmm * 1e6 / P, 3),
                              "torch_loop_chain_only_on_its_positions": round(per_loop, 1)},
          "path_accuracy": round(accuracy, 4), "largest_error_over_mass": worst,
          "note": "the torch loop ran on its positions only; nothing is extrapolated to the whole sequence"}, a.out)


if __name__ == "__main__":
    main()
