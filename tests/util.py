"""Seeded input generators shared by the CPU and GPU tests (NumPy only), and the tests' own reader of the C ABI's header."""
import ctypes
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bear_hip.h")


def abi_header(path=HEADER):
    """(BEAR_ABI_VERSION, {function: (restype, [argtypes])}) as ``path`` declares them, in ctypes terms.  Written apart from the
    reader of ``bear_amd._lib`` on purpose (the tests hold that one to this one): one pattern for a whole declaration, the
    parameter's type from its first word."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    scalar = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
              "double": ctypes.c_double}
    result = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "const char *": ctypes.c_char_p}

    def ctype(param):
        if "**" in param.replace(" ", ""):
            return ctypes.POINTER(ctypes.c_void_p)
        if "*" in param:
            return ctypes.c_char_p if re.fullmatch(r"\s*const\s+char\s*\*\s*path\s*", param) else ctypes.c_void_p
        return scalar[param.split()[0]]
    sigs = {}
    for res, name, params in re.findall(r"^(int|uint64_t|const char \*) ?(bear_[a-z0-9_]+)\(([^()]*)\);", src, flags=re.M):
        sigs[name] = (result[res], [] if params.strip() == "void" else [ctype(q) for q in params.split(",")])
    assert sorted(sigs) == sorted(set(re.findall(r"\b(bear_[a-z0-9_]+)\s*\(", src))), "a declaration this reader does not understand"
    return int(re.search(r"#define BEAR_ABI_VERSION (\d+)", src).group(1)), sigs


def stream_entries(path=HEADER):
    """The functions ``path`` declares with ``void *stream`` as their last parameter, in the header's order."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    decls = re.findall(r"^(?:int|uint64_t|const char \*) ?(bear_[a-z0-9_]+)\(([^()]*)\);", src, flags=re.M)
    return [name for name, params in decls if " ".join(params.split(",")[-1].split()) == "void *stream"]


def sparse_table(n, seed=0, lam_scale=1.0):
    """NumPy twin (same recipe, not the same bits) of the 'k=13 sparse' synthetic table."""
    rng = np.random.default_rng(seed)
    lam = np.exp(0.5 + 1.5 * rng.standard_normal(n)) * lam_scale
    w = -np.log(rng.random((n, 4))) * rng.random((n, 4)) ** (10 / 3)
    p = w / w.sum(1, keepdims=True) * (1 - 1 / 150)
    p = np.concatenate([p, np.full((n, 1), 1 / 150)], 1)
    train = rng.poisson(lam[:, None] * p).astype(np.uint32)
    test = rng.poisson(lam[:, None] * p / 3).astype(np.uint32)
    ref = rng.poisson(0.02 * lam[:, None] * p).astype(np.uint32)
    ref[:, 4] = 0
    return train, test, ref


def dense_table(n, seed=0):
    rng = np.random.default_rng(seed)
    lam = 1e4 * np.exp(rng.random(n) * np.log(30))
    p = rng.dirichlet(np.full(5, 2.0), size=n)
    train = rng.poisson(lam[:, None] * p).astype(np.uint32)
    ref = rng.poisson(1e-3 * lam[:, None] * p).astype(np.uint32)
    ref[:, 4] = 0
    return train, ref


def mixed_heavy_table(n=6000, seed=1):
    """A sparse table with ~6 % of its rows replaced by dense ones: full tiles (1664 contexts) that each hold several times more
    large-count cells and large-total rows than a tile keeps inside (PLN_HCAP = 128), many of them among the contexts a thread
    meets in its second pass (>= 1024 of the tile) -- the in-tile lists AND the plan's global lists fill.  (train, ref)."""
    train, _, ref = sparse_table(n, 5, lam_scale=1.0)
    dense, _ = dense_table(n, 7)
    m = np.random.default_rng(seed).random(n) < 0.06
    train[m] = dense[m]
    return train, ref


def prior_rows(n, seed=0, conc=1.0):
    rng = np.random.default_rng(seed + 1000)
    return rng.dirichlet(np.full(5, conc), size=n)


def edge_table(seed=0):
    """Rows that force every branch: all-zero, single transition, product/Stirling boundary,
    huge counts (uint32 range), one-hot rows."""
    rng = np.random.default_rng(seed)
    rows = [
        [0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 1], [1, 1, 1, 1, 1],
        [16, 0, 0, 0, 0], [17, 0, 0, 0, 0], [0, 16, 1, 0, 0], [8, 8, 0, 0, 1],
        [15, 16, 17, 18, 19], [100, 0, 3, 0, 0], [1000, 2000, 3000, 4000, 5],
        [4000000000, 0, 0, 0, 0], [4000000000, 4000000000, 4000000000, 4000000000, 100000],
        [254715, 3, 0, 1, 0], [0, 0, 65, 0, 0], [2, 0, 0, 31, 33],
    ]
    extra = rng.integers(0, 40, size=(48, 5))
    return np.asarray(rows + extra.tolist(), dtype=np.uint32)


U32_MAX = 4294967295


def edge_table_wide(W, seed=0):
    """Count rows of width W that force every branch of the wide kernels: no counts; one count in the first and in the last letter
    (the top bit of the non-zero mask); every cell 1; every cell 2^32 - 1 (a row total above 2^32); cells at the product / Stirling
    switch (16, 17) and above it (24, 25); cells of 1e5 to 3e6; random sparse and dense fills."""
    rng = np.random.default_rng(seed)
    z = np.zeros(W, np.int64)

    def one(b, v):
        r = z.copy()
        r[b] = v
        return r

    rows = [z, one(0, 1), one(W - 1, 1), np.ones(W, np.int64), np.full(W, U32_MAX), one(W - 1, U32_MAX), one(0, U32_MAX)]
    for v in (16, 17, 24, 25):
        rows += [np.full(W, v), one(v % W, v), one(W - 1, v)]
    rows.append(np.resize([16, 17, 24, 25, 0], W))
    rows.append(np.resize([0, 25, 1, 16, 24, 17], W))
    rows.append(rng.integers(100_000, 3_000_001, W))
    rows.append(np.where(rng.random(W) < 0.3, rng.integers(100_000, 3_000_001, W), 0))
    r = z.copy()
    r[W - 1], r[0] = U32_MAX, 1
    rows.append(r)
    for _ in range(12):                                           # random fill: sparse, dense, mixed magnitudes
        p = rng.choice([0.1, 0.5, 1.0])
        v = rng.integers(1, rng.choice([3, 40, 1000]), W)
        rows.append(np.where(rng.random(W) < p, v, 0))
    return np.asarray(rows, dtype=np.uint32)


PRIOR_KINDS = ("softmax", "onehot", "tiny", "scaled")


def prior_rows_wide(n, W, kind, seed=0):
    """Prior rows [n, W]: 'softmax' (normalised, spread over ~3 orders of magnitude), 'onehot' (one cell 1, the others exactly 0),
    'tiny' (softmax rows with cells of 1e-300 and 5e-324, the smallest subnormal), 'scaled' (softmax rows times 0.5 .. 3: not
    normalised)."""
    rng = np.random.default_rng(seed + 7919)
    z = rng.normal(size=(n, W)) * 2.0
    f = np.exp(z - z.max(1, keepdims=True))
    f /= f.sum(1, keepdims=True)
    if kind == "softmax":
        return f
    if kind == "onehot":
        f = np.zeros((n, W))
        hot = rng.integers(0, W, n)
        hot[:2] = [0, W - 1][:n]
        f[np.arange(n), hot] = 1.0
        return f
    if kind == "tiny":
        u = rng.random((n, W))
        f[u < 0.15] = 1e-300
        f[u > 0.85] = 5e-324
        return f
    if kind == "scaled":
        return f * rng.uniform(0.5, 3.0, (n, 1))
    raise ValueError(kind)


def tile_rows(table, n, seed=0):
    """n rows drawn from ``table``: every row of it first (in a seeded order), then repeats -- so that the edge rows land in every
    position of a tile."""
    rng = np.random.default_rng(seed)
    idx = np.r_[rng.permutation(len(table)), rng.integers(0, len(table), max(0, n - len(table)))][:n]
    return np.ascontiguousarray(table[idx])


def wide_scale_table(n, W, dense=False, seed=0):
    """A large seeded count table of width W (vectorised: no k-mer strings).  Sparse: ~15 % non-zero cells of Poisson counts, a
    few rows with counts of 1e5 .. 3e6, ~4 % empty rows; dense: every cell non-zero, counts up to ~3e4."""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(0.5, 40.0, (n, 1))
    if dense:
        c = rng.poisson(lam * rng.uniform(1.0, 800.0, (n, 1)), (n, W)) + 1
    else:
        c = np.where(rng.random((n, W)) < 0.15, rng.poisson(lam, (n, W)), 0)
        big = rng.choice(n, max(1, n // 5000), replace=False)
        c[big, rng.integers(0, W, big.size)] = rng.integers(100_000, 3_000_000, big.size)
        c[rng.choice(n, max(1, n // 24), replace=False)] = 0
    return c.astype(np.uint32)
