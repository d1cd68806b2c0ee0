"""Times the width-5 convolutional head (kernels_cnn.h) at lag 13, filter width 8 on 1e7 contexts:

  * cnn_forward and cnn_backward on random rows and on k-mer-sorted rows;
  * cnn_backward in the 64-context form (BEAR_CNN_BACKWARD=1) on the random rows;
  * the training step (net_cnn_train_reduce) on the table bear_net.train keeps resident -- k-mer order, contexts without training
    counts left out -- with prefix levels and window tables attached, and the forward pass over the same plan.

Device events after a warm-up call, three repetitions per figure.  One JSON line per figure, with the library's path and the
commit, printed and appended to --out.  One library per process (BEAR_AMD_LIB picks it): to hold one build against another, run
the two alternately, each in a fresh process per round.

    python scripts/cnn_time.py [--rows 1e7] [--out profiles/cnn_time.jsonl] [--tag new] [--commit 8d71244]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bear_amd import _lib, ar_funcs, kernels  # noqa: E402

LAG, FW, REPS = 13, 8, 3


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def kmer_sorted(codes):
    key = torch.zeros(codes.shape[0], dtype=torch.int64, device=codes.device)
    for l in range(codes.shape[1]):
        key = key * 6 + codes[:, l].to(torch.int64)
    return torch.argsort(key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_time.jsonl"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--commit", default=None, help="where the tree has no .git")
    a = ap.parse_args()
    n, dev = int(a.rows), torch.device("cuda", 0)
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    base = {"lib": _lib.LIB_PATH, "commit": commit or None, "tag": a.tag, "rows": n, "lag": LAG, "filter_width": FW}

    def emit(what, ms, **more):
        line = json.dumps(dict(base, what=what, ms=round(ms, 4), **more))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")

    gen = torch.Generator(dev).manual_seed(20211012)
    codes = torch.randint(0, 4, (n, LAG), dtype=torch.int8, device=dev, generator=gen)
    _, params = ar_funcs.make_ar_func_cnn(LAG, 4, filter_width=FW, device=dev, generator=torch.Generator(dev).manual_seed(10))
    flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
    g = torch.randn(n, 5, dtype=torch.float64, device=dev, generator=gen)
    order = kmer_sorted(codes)
    for name, packed in (("random", kernels.pack_kmers(codes)), ("sorted", kernels.pack_kmers(codes[order].contiguous()))):
        prior, t1 = kernels.cnn_forward(packed, flat, LAG, FW)
        emit("cnn_forward/" + name, timed(lambda: kernels.cnn_forward(packed, flat, LAG, FW)))
        emit("cnn_backward/" + name, timed(lambda: kernels.cnn_backward(packed, flat, LAG, FW, t1, prior, g)))
        if name == "random":
            os.environ["BEAR_CNN_BACKWARD"] = "1"
            emit("cnn_backward/random/64-context form", timed(lambda: kernels.cnn_backward(packed, flat, LAG, FW, t1, prior, g)))
            del os.environ["BEAR_CNN_BACKWARD"]
        del prior, t1, packed
    del g
    # the kept sorted table, as scripts/dev/cnn_levels_time.py builds it
    t = kernels.synth_counts(20211012, 0, n, dev, want=("train",))["train"]
    keep = (t[order] != 0).any(dim=1).nonzero().squeeze(1)
    tr = t[order].index_select(0, keep).contiguous()
    packed = kernels.pack_kmers(codes[order].index_select(0, keep).contiguous())
    del t, order, keep, codes
    kept = tr.shape[0]
    theta = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), flat]).contiguous()
    plan = kernels.Plan(tr, 5)
    bufs = kernels.cnn_step_buffers(kept, LAG, FW, dev)
    pk = torch.zeros(2 + flat.numel(), dtype=torch.float64, device=dev)
    levels = plan.attach_cnn_levels(packed, LAG, FW)
    shape = {"kept_rows": kept, "levels": levels, "level_rows": plan.cnn_level_rows(), "window_tables": plan.cnn_window_rows()}
    emit("net_cnn_train_reduce/levels+tables", timed(lambda: kernels.net_cnn_train_reduce(plan, packed, LAG, FW, theta, bufs, pk)), **shape)
    emit("cnn_forward/levels+tables", timed(lambda: kernels.cnn_forward(packed, flat, LAG, FW, plan=plan)), kept_rows=kept)


if __name__ == "__main__":
    main()
