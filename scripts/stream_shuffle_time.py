"""A streamed SHUFFLED epoch against a streamed epoch in file order (ResidentBatches with BEAR_AMD_STREAM=1): the same bear_net.train
call, linear AR function, over `batches` batches of `rows` synthetic contexts -- in file order (every batch uploaded through the
pinned ring) and shuffled (bear_shuffle_gather_host collects the batch's rows perm(a) .. perm(b - 1) with 16 host threads, then the
ring).  Two shapes: dna, k = 13, 4 x 1e7 contexts (the shape of scripts/stream_time.py) and prot, k = 5, 4 x 2e6 rows of 21.  Also the
host gather alone, and the gather kernel alone from device memory in GB/s of rows delivered (HIP events after settling launches).
One JSON line per measurement.
    python scripts/stream_shuffle_time.py [dna|prot|all] [epochs] [output file]"""
import itertools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from baseline_configs import _table
from prot_time import settle, synth

SHAPES = {"dna": dict(rows=10_000_000, batches=4, lag=13, width=5), "prot": dict(rows=2_000_000, batches=4, lag=5, width=21)}
PROT = "ARNDCEQGHILKMFPSTWYV"


def host_table(alphabet, shape, dev):
    n = shape["rows"] * shape["batches"]
    if alphabet == "dna":
        return _table(n, shape["lag"], dev, ("train",))
    counts = synth(n, dev, 1).cpu().numpy().view(np.uint32)[None]
    g = torch.Generator(dev).manual_seed(2)
    letters = torch.tensor(list(PROT.encode()), dtype=torch.uint8, device=dev)
    kmers = letters[torch.randint(0, 20, (n, shape["lag"]), device=dev, generator=g)].cpu().numpy()
    torch.cuda.empty_cache()
    return kmers, np.ascontiguousarray(counts)


def train_modes(alphabet, shape, data, epochs):
    """ms per optimizer step of the streamed loop, per mode."""
    from bear_amd import _train, ar_funcs, bear_net
    n = data.num_rows
    row_bytes = 4 * shape["width"] + shape["lag"]
    modes = (("streamed, file order", data), ("streamed, shuffled, host gather (16 threads)", data.shuffle(1)))
    keep = {k: os.environ.get(k) for k in ("BEAR_AMD_STREAM",)}
    os.environ["BEAR_AMD_STREAM"] = "1"
    try:
        for rep in range(2):                    # the modes in turn, twice: the spread next to the difference
            for name, d in modes:
                torch.manual_seed(1)
                loss = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bear_net.train(d.repeat(epochs), n, epochs, 0, alphabet, shape["lag"], ar_funcs.make_ar_func_linear, {}, 0.01, "Adam", False,
                               loss_save=loss)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                lr = dict(_train.LAST_RUN)
                assert lr["streaming"]
                per_step = lr["loop_ms"] / max(lr["loop_steps"], 1)
                yield {"what": "train", "alphabet": alphabet, "mode": name, "visit": rep, "rows_per_batch": shape["rows"],
                       "batches_per_epoch": shape["batches"], "epochs": epochs, "lag": shape["lag"], "width": shape["width"],
                       "host_bytes_per_context": row_bytes, "loop_ms_per_step": round(per_step, 3), "loop_steps": lr["loop_steps"],
                       "host_to_device_GBps_over_the_loop": round(shape["rows"] * row_bytes / per_step / 1e6, 2),
                       "train_call_wall_s": round(wall, 3), "elbo_last": loss[-1]}
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def gather_alone(alphabet, shape, data, dev):
    """The gather kernel by itself from device memory, and the host gather by itself: one batch's rows of the count column and of
    the k-mers."""
    from bear_amd import kernels
    n_out = shape["rows"]
    for what, array, dtype in (("counts", data.counts[0].view(np.int32), torch.int32), ("kmers", data.kmers, torch.uint8)):
        row_bytes = array.nbytes // array.shape[0]
        src = torch.from_numpy(array).to(dev)
        out = torch.empty((n_out,) + array.shape[1:], dtype=dtype, device=dev)
        firsts = [k * n_out for k in range(shape["batches"])]
        fn = lambda: [kernels.shuffle_rows_range(src, a, n_out, 1, out=out) for a in firsts]   # noqa: E731
        settle(fn, cap_s=2.0)
        best = float("inf")
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / len(firsts))
        yield {"what": "gather kernel alone", "alphabet": alphabet, "column": what, "source": "device memory", "row_bytes": row_bytes,
               "rows_out": n_out, "table_rows": array.shape[0], "ms": round(best, 3),
               "GBps_rows_delivered": round(n_out * row_bytes / best / 1e6, 2)}
        del src, out
        t0 = time.perf_counter()
        kernels.shuffle_gather_host(array, 0, n_out, 1, n_threads=16)
        t_host = time.perf_counter() - t0
        yield {"what": "host gather alone (16 threads)", "alphabet": alphabet, "column": what, "row_bytes": row_bytes, "rows_out": n_out,
               "ms": round(t_host * 1e3, 3), "GBps_rows_delivered": round(n_out * row_bytes / t_host / 1e9, 2)}


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    path = sys.argv[3] if len(sys.argv) > 3 else None
    from bear_amd import dataloader
    dev = torch.device("cuda", 0)
    fh = open(path, "a") if path else None
    for alphabet in (("dna", "prot") if which == "all" else (which,)):
        shape = SHAPES[alphabet]
        kmers, counts = host_table(alphabet, shape, dev)
        data = dataloader.CountDataset(kmers, counts, alphabet, shape["rows"])
        for line in itertools.chain(gather_alone(alphabet, shape, data, dev), train_modes(alphabet, shape, data, epochs)):
            text = json.dumps(line)
            print(text, flush=True)
            if fh:
                fh.write(text + "\n")
                fh.flush()
        del data, kmers, counts
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
