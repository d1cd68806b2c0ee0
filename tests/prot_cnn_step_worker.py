"""Worker of tests/test_prot_cnn_step_gpu.py: one rank of a 2-process run of bear_net.train with the convolutional AR function on a
protein table.  Launched by ``python -m torch.distributed.run``; both ranks share cuda:0 (BEAR_AMD_DEVICE=0) and reduce over gloo
(BEAR_AMD_DIST_BACKEND=gloo).  Each rank loads the whole table; CountDataset.rank_pieces deals the rows of every batch."""
import json
import os
import sys

ROOT = os.environ["BEAR_ROOT"]
sys.path.insert(0, ROOT)

import numpy as np
import torch

from bear_amd import ar_funcs, bear_net, dataloader, dist, kernels


def main():
    rank, world = dist.init_from_env()
    assert world == 2 and torch.cuda.current_device() == 0
    saved = np.load(os.environ["BEAR_RESTART"])
    restart = [saved["p%d" % i] for i in range(len(saved.files))]
    data = dataloader.dataloader(os.environ["BEAR_TABLE"], "prot", 150, 3)
    calls = []
    real_reduce, real_rows = kernels.net_cnn_train_reduce_wide, kernels.cnn_forward_wide
    kernels.net_cnn_train_reduce_wide = lambda *a, **kw: (calls.append("wide"), real_reduce(*a, **kw))[1]
    kernels.cnn_forward_wide = lambda *a, **kw: (calls.append("rows"), real_rows(*a, **kw))[1]
    out = {}
    for train_ar in (False, True):
        del calls[:]
        ls = []
        p, _, _ = bear_net.train(data.repeat(6), data.num_rows, 6, 0, "prot", 4, ar_funcs.make_ar_func_cnn, {"filter_width": 3}, 0.01, "Adam",
                                 train_ar, params_restart=restart, loss_save=ls)
        out["ar" if train_ar else "bear"] = {"loss": ls, "params": [x.detach().cpu().numpy().tolist() for x in p],
                                             "step_fns": "/".join(sorted(set(calls)))}
    if rank == 0:
        with open(os.environ["BEAR_OUT"], "w") as fh:
            json.dump(out, fh)
    dist.shutdown()


if __name__ == "__main__":
    main()
