"""Times one optimizer step of bear_net.train with the convolutional AR function on a protein table: the fused form (two launches,
kernels_cnn_wide.h: cnn_wide_head_dm_kernel + cnn_wide_backward_kernel<true>, Adam in the second) against the path it replaces
(BEAR_AMD_UNFUSED_CNN_WIDE=1: cnn_wide_forward_kernel, dm_wide_kernel with gradient rows and cnn_wide_backward_kernel<false> under torch
autograd, run_autograd_steps -- the code of the commit before the fused form, whose kernels keep their bits: scripts/dev/wide_bits.py).

One batch = the table; the step is replayed from a HIP graph where the path captures one (the former path runs eagerly above
BEAR_AMD_GRAPH_MAX_ROWS = 4 Mi rows).  The figure is the device time of the loop's later steps as run_device_steps measures it (HIP
events on the launch stream after the first quarter of the steps, _train.LAST_RUN), after a warm-up run of each path (allocator,
clocks).  The two paths alternate in one process, three rounds; best and worst of each are reported, and the rule of
scripts/prot_ref_time.py: the new path's best time lies within or below the former path's best-to-worst spread (``new_not_slower``).

    python scripts/prot_cnn_step_time.py [--out profiles/prot_cnn_step_time.jsonl] [--rows 1365,1e5,1e6,1e7] [--shapes 5/3,12/8] [--tag T]

Appends one JSON line per figure to --out (and prints it).  --tag names the tree in every line: copied into a checkout of the commit
before the fused form, where the switch does nothing, the script times that commit's path twice ("new" and "former" alike), which
is how profiles/prot_cnn_step_time.jsonl holds both commits from one box."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bear_amd import _train, ar_funcs, bear_net, core, dataloader  # noqa: E402
from prot_linear_step_time import compare, emit  # noqa: E402
from prot_time import synth  # noqa: E402

W = 21


def time_train(out, n, lag, fw, dev, tag):
    g = torch.Generator(dev).manual_seed(5)
    letters = torch.tensor([ord(c) for c in core.alphabets_en["prot"][:20]], dtype=torch.uint8, device=dev)
    kmers = letters[torch.randint(0, 20, (n, lag), device=dev, generator=g)]
    data = dataloader.DeviceCountDataset(kmers, synth(n, dev, 1)[None].contiguous(), "prot", n)
    epochs = max(16, min(400, int(2e7 // n)))
    info = {}

    def step_ms(path):
        if path == "former":
            os.environ["BEAR_AMD_UNFUSED_CNN_WIDE"] = "1"
        try:
            torch.manual_seed(1)
            bear_net.train(data.repeat(epochs), n, epochs, 0, "prot", lag, ar_funcs.make_ar_func_cnn, {"filter_width": fw}, 0.01, "Adam", False)
        finally:
            os.environ.pop("BEAR_AMD_UNFUSED_CNN_WIDE", None)
        run = _train.LAST_RUN
        info["graph_" + path] = bool(run["graph"])
        return run["timed_ms"] / max(run["timed_steps"], 1)
    for path in ("new", "former"):
        step_ms(path)                            # warm-up: allocator, algorithm choices, the clocks
    base = {"tree": tag, "rows": n, "lag": lag, "filter_width": fw, "width": W, "batch": n, "steps": epochs}
    compare(out, base, "bear_net_cnn_train_step", {"new": None, "former": None}, step_ms)
    emit(out, dict(base, what="bear_net_cnn_train_step_graph", **info))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1365,1e5,1e6,1e7")
    ap.add_argument("--shapes", default="5/3,12/8")
    ap.add_argument("--tag", default="branch")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for n in [int(float(x)) for x in a.rows.split(",")]:
        for lag, fw in [tuple(int(v) for v in x.split("/")) for x in a.shapes.split(",")]:
            time_train(a.out, n, lag, fw, dev, a.tag)


if __name__ == "__main__":
    main()
