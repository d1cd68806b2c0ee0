"""Host-side: throughput of the threaded count-table reader (bear_parse_counts_tsv), of the row counter (bear_count_rows), of the
writer (bear_write_counts_tsv) and of one rank of a world = 4 sharded read (bear_parse_counts_tsv_shard), by thread count."""
import ctypes, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bear_amd import _lib
rng = np.random.default_rng(0)
n, lag = int(float(sys.argv[1])) if len(sys.argv) > 1 else 8_000_000, 13
letters = np.frombuffer(b"ACGT", dtype=np.uint8)
kmers = letters[rng.integers(0, 4, size=(n, lag))]
counts = rng.poisson(1.5, size=(3, n, 5)).astype(np.uint32)
L = _lib.lib(); path = "/tmp/bear_parse_time.tsv"; path2 = "/tmp/bear_parse_time_out.tsv"
L.bear_write_counts_tsv(path.encode(), kmers.ctypes.data, counts.ctypes.data, n, lag, 3, 0, 1, 0)
km = np.ones((n, lag), dtype=np.uint8); cn = np.ones((3, n, 5), dtype=np.uint32); got = ctypes.c_uint64(); rows = ctypes.c_uint64()
mb = os.path.getsize(path) / 1e6
# rank 1 of 4, batches of 4096 rows: its rows by dist.shard_rows' rule
B, W, R = 4096, 4, 1
g = np.arange(n); a = g // B * B; m = np.minimum(B, n - a); base, extra = m // W, m % W
lo = R * base + np.minimum(R, extra); mine = np.flatnonzero((g - a >= lo) & (g - a < lo + base + (R < extra)))
kms = np.ones((len(mine), lag), dtype=np.uint8); cns = np.ones((3, len(mine), 5), dtype=np.uint32)


def best(call):
    t = []
    for _ in range(2):
        t0 = time.time(); st = call(); t.append(time.time() - t0)
        assert st == 0
    return min(t)


for th in ("1", "2", "4", "8", "16", "32"):
    os.environ["BEAR_PARSE_THREADS"] = th
    t = best(lambda: L.bear_parse_counts_tsv(path.encode(), 3, lag, n, km.ctypes.data, cn.ctypes.data, ctypes.byref(got)))
    assert np.array_equal(cn, counts)
    print(th, "threads: %.3f s  %.0f MB/s  %.1f Mrows/s" % (t, mb / t, n / t / 1e6), flush=True)
    t = best(lambda: L.bear_count_rows(path.encode(), ctypes.byref(rows)))
    assert rows.value == n
    print(th, "threads count_rows: %.3f s  %.0f MB/s" % (t, mb / t), flush=True)
    t = best(lambda: L.bear_write_counts_tsv(path2.encode(), kmers.ctypes.data, counts.ctypes.data, n, lag, 3, 0, 1, 0))
    assert os.path.getsize(path2) == os.path.getsize(path)
    print(th, "threads write: %.3f s  %.0f MB/s  %.1f Mrows/s" % (t, mb / t, n / t / 1e6), flush=True)
    t = best(lambda: L.bear_parse_counts_tsv_shard(path.encode(), 3, lag, 0, 0, n, B, R, W, len(mine), kms.ctypes.data, cns.ctypes.data,
                                                   ctypes.byref(got), ctypes.byref(rows)))
    assert got.value == len(mine) and rows.value == n and np.array_equal(cns, counts[:, mine]) and np.array_equal(kms, kmers[mine])
    print(th, "threads shard 1/4: %.3f s  %.0f MB/s  %.1f Mrows/s" % (t, mb / t, len(mine) / t / 1e6), flush=True)
os.remove(path); os.remove(path2)
print("cpus", os.cpu_count(), len(os.sched_getaffinity(0)))
