"""What the CPU and GPU tests of the two-sample Bayes factors share (bear_two_sample_f64, bear_amd.hypothesis): the oracle -- the
formulas of include/bear_hip.h written out with mpmath at 50 digits, value and L1 mass of the terms, row by row -- its SciPy
twin for whole tables, the rows that force every path of the kernel, and the statistical case (Markov chains, their sequences,
a host count of their transitions)."""
import functools

import mpmath
import numpy as np

HS = np.array([1e-6, 0.7, 1e6])            # three h values in 1e-6 .. 1e6
VANS = np.array([0.1, 1.0, 10.0])
RTOL = 1e-11                               # of each output's L1 term mass: tests/test_marg_gpu.py RTOL, the same item routine and terms
U32_MAX = 0xFFFFFFFF


def concentrations(prior_row, hs, vans, W):
    """Per model the float64 concentrations [W] and their total A, formed as the entry forms them: ``prior * (1.0 / h)`` resp. ``van``,
    added in the order of the cells."""
    out = []
    for h in hs:
        out.append(np.asarray(prior_row, dtype=np.float64) * np.float64(1.0 / h))
    for v in vans:
        out.append(np.full(W, float(v)))
    totals = []
    for al in out:
        A = np.float64(0.0)
        for x in al:
            A = A + x
        totals.append(A)
    return out, totals


@functools.lru_cache(maxsize=1 << 14)
def _lg(x, n):
    """lgamma(x + n) of a float64 x and an integer n, at the working precision (called at 50 digits only: the three T of a row
    share lgamma(A) and every lgamma(alpha_j))."""
    return mpmath.loggamma(mpmath.mpf(x) + n)


def _T(alpha, A, c):
    """(value, mass) of T(c) as mpmath numbers: the brackets lgamma(A) - lgamma(A + n) and lgamma(alpha_j + c_j) - lgamma(alpha_j)."""
    n = int(sum(int(x) for x in c))
    if n == 0:
        return mpmath.mpf(0), mpmath.mpf(0)
    terms = [_lg(float(A), 0) - _lg(float(A), n)]
    terms += [_lg(float(alpha[j]), int(c[j])) - _lg(float(alpha[j]), 0) for j in range(len(c)) if int(c[j])]
    return mpmath.fsum(terms), mpmath.fsum(abs(t) for t in terms)


def oracle_rows(a, b, prior, hs, vans):
    """Row by row: ``val``, ``mass`` = object arrays [N, M, 4] of mpmath numbers {T(a), T(b), T(a + b), B_k} and the L1 masses of
    their terms (B_k's: all three), and ``ar``, ``ar_mass`` [N, 2] = {sum a_j log prior_j, the same of b} (zeros without prior)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    N, W = a.shape
    M = len(hs) + len(vans)
    val, mass = np.empty((N, M, 4), dtype=object), np.empty((N, M, 4), dtype=object)
    ar, ar_mass = np.empty((N, 2), dtype=object), np.empty((N, 2), dtype=object)
    with mpmath.workdps(50):
        for k in range(N):
            ca, cb = [int(x) for x in a[k]], [int(x) for x in b[k]]
            cab = [x + y for x, y in zip(ca, cb)]
            alphas, totals = concentrations(prior[k] if prior is not None else np.zeros(W), hs, vans, W)
            for m in range(M):
                ta, tb, tab = (_T(alphas[m], totals[m], c) for c in (ca, cb, cab))
                val[k, m] = [ta[0], tb[0], tab[0], (ta[0] + tb[0]) - tab[0]]
                mass[k, m] = [ta[1], tb[1], tab[1], ta[1] + tb[1] + tab[1]]
            for s, c in enumerate((ca, cb)):
                terms = [c[j] * mpmath.log(mpmath.mpf(float(prior[k, j]))) for j in range(W) if c[j]] if prior is not None else []
                ar[k, s], ar_mass[k, s] = mpmath.fsum(terms), mpmath.fsum(abs(t) for t in terms)
    return val, mass, ar, ar_mass


def oracle_sums(rows, idx=None):
    """The table ``base[idx]`` (``rows`` = ``oracle_rows(base...)``; None: the base itself) summed at 50 digits -> float64
    ``(out [M, 4], out_mass [M, 4], ar [2], ar_mass [2])``."""
    val, mass, ar, ar_mass = rows
    mult = np.bincount(idx, minlength=val.shape[0]) if idx is not None else np.ones(val.shape[0], dtype=np.int64)
    with mpmath.workdps(50):
        def total(x):
            flat = x.reshape(x.shape[0], -1)
            s = [mpmath.fsum(int(mult[k]) * flat[k, q] for k in range(flat.shape[0]) if mult[k]) for q in range(flat.shape[1])]
            return np.array([float(v) for v in s]).reshape(x.shape[1:])
        return total(val), total(mass), total(ar), total(ar_mass)


def unique_rows(a, b, prior):
    """``(first, inverse)``: the distinct (a, b, prior) rows of a table (``first``: a row number of each) and every row's number
    among them -- a sparse table under a uniform prior is a few distinct rows many times, and the oracle is paid per distinct row."""
    key = np.concatenate([a.astype(np.float64), b.astype(np.float64), prior], 1)           # (uint32 is exact in float64)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return first, inverse.reshape(-1)


def as_float(x):
    return np.array([float(v) for v in x.reshape(-1)]).reshape(x.shape)


def scipy_sums(a, b, prior, hs, vans):
    """The SciPy twin for whole tables: float64 ``(out [M, 4], ar [2] or None)``, vectorised over the rows."""
    from scipy.special import gammaln
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    N, W = a.shape
    out = []
    for m in range(len(hs) + len(vans)):
        al = prior * (1.0 / hs[m]) if m < len(hs) else np.full((N, W), float(vans[m - len(hs)]))
        A = al.sum(1)

        def T(c):
            n = c.sum(1)
            cell = np.where(c > 0, gammaln(al + c) - gammaln(al), 0.0).sum(1)
            return np.where(n > 0, gammaln(A) - gammaln(A + n) + cell, 0.0)
        ta, tb, tab = T(a), T(b), T(a + b)
        out.append([ta.sum(), tb.sum(), tab.sum(), ((ta + tb) - tab).sum()])
    ar = None
    if prior is not None:
        ar = np.array([np.where(c > 0, c * np.log(np.where(c > 0, prior, 1.0)), 0.0).sum() for c in (a, b)])
    return np.array(out), ar


# ------------------------------------------------------------------------------------------- rows of every kind
def base_rows(W, seed=0):
    """``(a, b, prior)`` uint32 [n, W] x 2 and float64 [n, W]: rows of every kind the kernel tells apart -- both empty; only a; only
    b; disjoint letters; equal rows; counts of 1; counts at and above the product / Stirling switch of the item routine (31 / 32),
    alone and pooled across it; large counts; 0xFFFFFFFF in both columns of one cell and of all cells (pooled beyond 2^32, the row
    total beyond 2^36); random sparse and dense fills -- with random normalised prior rows.  Row 0 holds both samples."""
    rng = np.random.default_rng(1000 + W + seed)
    z = np.zeros(W, np.int64)

    def cells(**kw):
        r = z.copy()
        for j, v in kw.items():
            r[int(j[1:]) % W] = v
        return r
    even, odd = np.arange(W) % 2 == 0, np.arange(W) % 2 == 1
    pairs = [
        (cells(c0=3, c2=1, c4=40), cells(c0=1, c1=2, c4=7)),                   # row 0: both samples, shared and unshared cells
        (z, z),                                                                # both empty
        (cells(c1=5, c3=1), z), (z, cells(c0=2, c4=33)),                       # only a, only b
        (np.where(even, 3, 0), np.where(odd, 2, 0)),                           # disjoint letters
        (cells(c0=4, c2=9, c4=1), cells(c0=4, c2=9, c4=1)),                    # equal rows
        (cells(c0=1), cells(c0=1)), (cells(c4=1), cells(c1=1)), (np.ones(W, np.int64), np.ones(W, np.int64)),      # counts of 1
        (cells(c0=16), cells(c0=16)), (cells(c1=31), cells(c1=1)), (cells(c2=32), cells(c2=31)), (cells(c3=17), cells(c3=15)),
        (cells(c0=33, c1=100), cells(c0=1000, c1=64)), (np.full(W, 40), np.full(W, 50)),                           # the Stirling path
        (rng.integers(100_000, 3_000_001, W), rng.integers(100_000, 3_000_001, W)),
        (cells(c2=U32_MAX), cells(c2=U32_MAX)),                                # one cell: pooled 2^33 - 2
        (np.full(W, U32_MAX), np.full(W, U32_MAX)),                            # all cells
        (np.full(W, U32_MAX), z), (cells(c4=U32_MAX, c0=1), cells(c4=1, c0=U32_MAX)),
    ]
    for _ in range(20):                                                        # random fills: sparse, dense, mixed magnitudes
        rows = []
        for _ in range(2):
            p = rng.choice([0.1, 0.4, 1.0])
            rows.append(np.where(rng.random(W) < p, rng.integers(1, rng.choice([3, 40, 1000]), W), 0))
        pairs.append(tuple(rows))
    a = np.asarray([p[0] for p in pairs], dtype=np.uint32)
    b = np.asarray([p[1] for p in pairs], dtype=np.uint32)
    prior = rng.dirichlet(np.full(W, 0.5), size=len(pairs)) + 1e-7
    prior /= prior.sum(1, keepdims=True)
    return a, b, prior


def table_index(n_base, n, seed=0):
    """Row numbers [n] into the base: row 0 first, then every other row in a seeded order, then repeats -- the rows of every kind land
    in every position of a tile."""
    rng = np.random.default_rng(seed)
    return np.r_[0, 1 + rng.permutation(n_base - 1), rng.integers(0, n_base, max(0, n - n_base))][:n]


# ------------------------------------------------------------------------------------------- the statistical case
LETTERS = {"dna": "ACGT", "prot": "ARNDCEQGHILKMFPSTWYV"}
STAT_CASE = {"dna": (2, (1, 3, 5)), "prot": (1, (1, 2, 3))}      # order of the chains, lags (tests/test_two_sample_cpu.py says why)


def chain(seed, alphabet="dna", order=2):
    """Transition rows [A^order, A] of a Markov chain, each drawn from Dirichlet(0.7)."""
    A = len(LETTERS[alphabet])
    return np.random.default_rng(seed).dirichlet(np.full(A, 0.7), size=A ** order)


def sample_seqs(P, seed, alphabet="dna", n_seqs=100, length=120, order=2):
    letters = LETTERS[alphabet]
    A = len(letters)
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(n_seqs):
        s = [int(x) for x in rng.integers(0, A, order)]
        for _ in range(order, length):
            ctx = 0
            for x in s[-order:]:
                ctx = ctx * A + x
            s.append(int(rng.choice(A, p=P[ctx])))
        seqs.append("".join(letters[x] for x in s))
    return seqs


def count_host(seqs_a, seqs_b, lag, alphabet="dna"):
    """The two-column transition table of the sequences, counted on the host: every sequence padded with ``lag`` start symbols and
    one stop -> ``(a, b)`` uint32 [n, A + 1] over the contexts seen (sorted)."""
    letters = LETTERS[alphabet] + "]"
    table = {}
    for col, seqs in enumerate((seqs_a, seqs_b)):
        for s in seqs:
            t = "[" * lag + s + "]"
            for p in range(lag, len(t)):
                table.setdefault(t[p - lag:p], np.zeros((2, len(letters)), np.uint32))[col, letters.index(t[p])] += 1
    keys = sorted(table)
    both = np.stack([table[k] for k in keys]) if keys else np.zeros((0, 2, len(letters)), np.uint32)
    return np.ascontiguousarray(both[:, 0]), np.ascontiguousarray(both[:, 1])
