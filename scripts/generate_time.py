"""Times assemble.assemble_no_ends through the host loop (a closure ``counter=`` over a dictionary) and through the device path (a
DeviceCounter, kernels_generate.h), both in this process on the same table.

    python scripts/generate_time.py [--seeds 10] [--replicates 100] [--letters 1000] [--table-rows 1e6] [--lag 8]
                                    [--host-letters N] [--cases dna_bmm,dna_trained,prot_bmm] [--out profiles/generate_time.jsonl]

Three cases, every seed grown to the right by ``--letters`` letters in ``--replicates`` replicates: a BMM over a random dna table of
``--table-rows`` distinct lag-``--lag`` contexts (no more than 4^lag exist: at lag 8 the full 65 536), a trained lag-5 linear model
(``bear_lin_bear.cfg`` on the bundled table, two epochs) over that table, and a BMM over a random lag-5 protein table.  The host loop
is timed once, the device path is the best and worst of three calls after one untimed call; wall time around a synchronise.  The
host loop's table of sampled rows grows with every new k-mer and is copied at every step, so ``--host-letters`` may give it a
shorter flank; the line then holds both lengths, and letters per second of each path.  One JSON line per case is printed and
appended to ``--out``."""
import argparse
import configparser
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import assemble, core, dataloader, get_var_probs  # noqa: E402


def random_table(alphabet_name, lag, n_rows, seed):
    """``(k-mer strings, CountDataset)``: n_rows distinct random contexts (at most all of them) with sparse Poisson counts."""
    rng = np.random.default_rng(seed)
    letters = np.array(list(core.alphabets_en[alphabet_name][:-1]))
    A = len(letters)
    ids = np.unique(rng.integers(0, A ** lag, size=int(n_rows * 1.3))) if n_rows < A ** lag else np.arange(A ** lag)
    ids = np.sort(rng.permutation(ids)[:n_rows])
    digits = (ids[:, None] // A ** np.arange(lag - 1, -1, -1)[None, :]) % A
    kmers = ["".join(r) for r in letters[digits]]
    n = len(kmers)
    lam = np.exp(rng.random((n, 1)) * 5)
    counts = np.where(rng.random((n, A + 1)) < 0.4, rng.poisson(np.broadcast_to(lam, (n, A + 1))), 0).astype(np.uint32)
    kmer_bytes = np.frombuffer("".join(kmers).encode(), dtype=np.uint8).reshape(n, lag).copy()
    return kmers, dataloader.CountDataset(kmer_bytes, counts[None], alphabet_name, 100000)


def host_counter_of(kmers, counts):
    """The host look-up a user had: a dictionary over the table's k-mer strings (no_end: the stop column reads 0)."""
    row = {k: i for i, k in enumerate(kmers)}
    W = counts.shape[1]

    def counter(q):
        q = np.asarray(q)
        out = np.zeros((q.size, W))
        for i, k in enumerate(q.reshape(-1).tolist()):
            j = row.get(str(k))
            if j is not None:
                out[i] = counts[j]
        out[:, -1] = 0
        return out.reshape(q.shape + (W,))
    return counter


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def run_case(name, a, tmp):
    alphabet_name = "prot" if name.startswith("prot") else "dna"
    bear_path, van = None, 0.5
    if name == "dna_trained":
        from bear_amd.models import train_bear_net
        config = configparser.ConfigParser()
        config.read(os.path.join(ROOT, "bear_amd", "models", "config_files", "bear_lin_bear.cfg"))
        config["train"]["epochs"] = "2"
        config["general"]["out_folder"] = os.path.join(tmp, "model") + "*"
        config["test"]["test"] = "False"
        config["test"]["train_test"] = "False"
        assert train_bear_net.main(config) == 1
        bear_path, van = os.path.join(tmp, "model"), None
        lag, _, _, _, data = get_var_probs.load_bear(bear_path)
        kmers = [bytes(k).decode() for k in np.asarray(data.kmers)]
    else:
        lag = a.lag if alphabet_name == "dna" else 5
        kmers, data = random_table(alphabet_name, lag, int(a.table_rows), 1)
    host_counter = host_counter_of(kmers, np.asarray(data.counts[0]))
    dev_counter, setup_s = timed(lambda: get_var_probs.DeviceCounter.from_dataset(data, 0, no_end=True))
    rng = np.random.default_rng(2)
    letters = list(core.alphabets_en[alphabet_name][:-1])
    seeds = ["".join(rng.choice(letters, lag + 12)) for _ in range(a.seeds)]
    fa = os.path.join(tmp, name + ".fa")
    with open(fa, "w") as fh:
        fh.write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seeds)))

    def call(counter, n_letters):
        kw = dict(lag=lag, alphabet_name=alphabet_name) if bear_path is None else {}
        return assemble.assemble_no_ends(fa, [[0, n_letters]] * a.seeds, a.replicates, bear_path, None, van=van, counter=counter, seed=3,
                                         **kw)[0]
    call(dev_counter, a.letters)
    dev_times = []
    for _ in range(3):
        gen, t = timed(lambda: call(dev_counter, a.letters))
        dev_times.append(t)
    assert gen.shape == (a.seeds, a.replicates) and all(len(s) == lag + 12 + a.letters for s in gen.reshape(-1))
    line = {"call": "assemble_no_ends", "case": name, "alphabet": alphabet_name, "lag": lag, "table_rows": len(kmers), "seeds": a.seeds,
            "replicates": a.replicates, "letters": a.letters, "device_path_s": [round(min(dev_times), 4), round(max(dev_times), 4)],
            "device_counter_setup_s": round(setup_s, 4),
            "device_letters_per_s": round(a.seeds * a.replicates * a.letters / min(dev_times))}
    if a.host_letters > 0:
        host, host_s = timed(lambda: call(host_counter, a.host_letters))
        assert host.shape == gen.shape
        line.update({"host_letters": a.host_letters, "host_counter_path_s": round(host_s, 3),
                     "host_letters_per_s": round(a.seeds * a.replicates * a.host_letters / host_s)})
        if a.host_letters == a.letters:
            line["host_over_device"] = round(host_s / min(dev_times), 1)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--letters", type=int, default=1000)
    ap.add_argument("--host-letters", type=int, default=None, help="flank of the host loop (default: --letters; 0: skip it)")
    ap.add_argument("--table-rows", type=float, default=1e6)
    ap.add_argument("--lag", type=int, default=8)
    ap.add_argument("--cases", default="dna_bmm,dna_trained,prot_bmm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_time.jsonl"))
    a = ap.parse_args()
    if a.host_letters is None:
        a.host_letters = a.letters
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.cases.split(","):
            text = json.dumps(run_case(name, a, tmp))
            print(text, flush=True)
            with open(a.out, "a") as fh:
                fh.write(text + "\n")


if __name__ == "__main__":
    main()
