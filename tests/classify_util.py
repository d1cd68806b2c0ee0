"""What the CPU and GPU tests of the group classifier share (bear_score_groups_f64, bear_amd.classify): the oracle -- the formula of
include/bear_hip.h evaluated with mpmath at 50 digits, the leave-one-out group included --, the kernel case and the statistical
case.  Nothing here touches a device."""
import functools
from collections import Counter

import mpmath
import numpy as np

import two_sample_util as tu

RTOL = 1e-11                       # |got - want| <= RTOL * L1 mass: the bound of tests/test_marg_gpu.py for this family
HS = np.array([0.05, 3.0])
VANS = np.array([0.1, 1.0, 10.0])
K, G = 37, 3
# tests/test_marg_gpu.py's segments with 5000 random positions for its 70 000: empty in front, one transition, a k-mer seen with
# several letters, empty in the middle, one (row, letter) 3000 times (beyond the product / Stirling switch at 16 and one chunk of
# 2048), a segment over several chunks with positions that hold no transition, a short one, empty last
LENS = [0, 1, 9, 0, 3000, 5000, 41, 0]
OWN = [0, 0, -1, 2, 0, 2, 7, -1]   # the group that holds each segment: none, 0, 2 and an out-of-range 7 (treated as none)
LIMIT_ROWS = (5, 6)                # rows with entries at the counter's limit: no segment with an own group touches them


@functools.lru_cache(maxsize=None)
def _lg(x):
    return mpmath.loggamma(x)


def oracle(entries_of_segments, hs, vans, W, n_groups, own=None):
    """``(want, mass)`` float64 [n_seg, G, H + V].  Per segment a list of k-mers ``(c [G, W] integers, f [W] floats or None,
    {letter: q})``; per group and model ``a_j = f_j / h + c_j`` (BEAR) or ``van + c_j``, ``A = sum_j a_j``, ``n = sum_j q_j`` and the
    term ``lgamma(A) - lgamma(A + n) + sum_{q_j > 0} [lgamma(a_j + q_j) - lgamma(a_j)]``; in the segment's own group ``c_j - q_j``
    stands for ``c_j`` (NaN for the whole segment and group where that is negative).  mass: the absolute values of the brackets."""
    H, M = len(hs), len(hs) + len(vans)
    want, mass = (np.zeros((len(entries_of_segments), n_groups, M)) for _ in range(2))
    with mpmath.workdps(50):
        mpf = mpmath.mpf
        w = [1 / mpf(float(v)) for v in hs] + [mpf(float(v)) for v in vans]
        for s, entries in enumerate(entries_of_segments):
            mine = -1 if own is None or not 0 <= own[s] < n_groups else int(own[s])
            for g in range(n_groups):
                for m in range(M):
                    total, l1 = mpf(0), mpf(0)
                    for c, f, q in entries:
                        cg = [int(c[g][j]) - (q.get(j, 0) if g == mine else 0) for j in range(W)]
                        if min(cg) < 0:
                            total = mpf("nan")
                            break
                        a = [mpf(float(f[j])) * w[m] + cg[j] if m < H else w[m] + cg[j] for j in range(W)]
                        A, n = mpmath.fsum(a), sum(q.values())
                        terms = [_lg(A) - _lg(A + n)] + [_lg(a[j] + qj) - _lg(a[j]) for j, qj in q.items()]
                        total += mpmath.fsum(terms)
                        l1 += mpmath.fsum(abs(t) for t in terms)
                    want[s, g, m], mass[s, g, m] = float(total), float(l1)
    return want, mass


def log_post(log_marg, log_prior=None):
    """``log_marg [n, G, M] + log_prior [G]`` less its logsumexp over the groups, with mpmath at 50 digits -> float64 [n, G, M]."""
    n, n_groups, M = log_marg.shape
    prior = np.zeros(n_groups) if log_prior is None else np.asarray(log_prior, dtype=np.float64)
    out = np.zeros(log_marg.shape)
    with mpmath.workdps(50):
        for i in range(n):
            for m in range(M):
                joint = [mpmath.mpf(float(log_marg[i, g, m])) + mpmath.mpf(float(prior[g])) for g in range(n_groups)]
                top = max(joint)
                norm = top + mpmath.log(mpmath.fsum(mpmath.exp(x - top) for x in joint))
                out[i, :, m] = [float(x - norm) for x in joint]
    return out


# ------------------------------------------------------------------------------------------- the kernel case
def segment_entries(segment, train, prior, W):
    """The k-mers of ``oracle`` of one segment ``(rows, letters)``: the positions with a transition, whatever their order."""
    runs = {}
    for r, b in zip(segment[0].tolist(), segment[1].tolist()):
        if 0 <= r < len(train) and b < W:
            runs.setdefault(r, Counter())[b] += 1
    return [(train[r], None if prior is None else prior[r], q) for r, q in runs.items()]


def counts_of(segment, n_rows, W):
    """uint32 [n_rows, W]: how often the segment holds every transition."""
    out = np.zeros((n_rows, W), dtype=np.uint32)
    live = (segment[0] >= 0) & (segment[0] < n_rows) & (segment[1] < W)
    np.add.at(out, (segment[0][live], segment[1][live]), 1)
    return out


def kernel_case(W):
    """``(segments, train uint32 [K, G, W], prior [K, W])``: text-order (rows, letters) of every segment of LENS, as
    tests/test_marg_gpu.py builds them, and a table that holds every segment in its group of OWN."""
    rng = np.random.default_rng(300 + W)
    train = np.where(rng.random((K, G, W)) < 0.5, rng.poisson(20.0, (K, G, W)), 0).astype(np.uint32)
    train[[3, 17]] = 0                                     # k-mers no group has seen
    train[5, :, ::2] = 4294967295                          # entries at the counter's limit
    train[6] = 4294967295
    prior = rng.dirichlet(np.full(W, 0.5), size=K) + 1e-7
    segments = []
    for n, own in zip(LENS, OWN):
        if n == 1:
            rows, letters = np.array([3]), np.array([W - 1])
        elif n == 9:
            rows, letters = np.array([5, 5, 5, 5, 6, 6, 5, 2, 5]), np.array([0, 1, 0, W - 1, 2, 2, 1, 0, 0])
        elif n == 3000:
            rows, letters = np.full(n, 9), np.full(n, 2)
        else:
            rows, letters = rng.integers(0, K, n), rng.integers(0, W, n)
            u = rng.random(n)
            rows = np.where(u < 0.1, -1, rows)             # 10 % of the positions hold no transition (1 % by the row alone,
            letters = np.where((u < 0.09) | ((u >= 0.1) & (u < 0.11)), 0xFF, letters)      # another 1 % by the letter alone)
            if 0 <= own < G:
                rows = np.where(np.isin(rows, LIMIT_ROWS), rows + 2, rows)
        segments.append((rows.astype(np.int32), letters.astype(np.uint8)))
    for segment, own in zip(segments, OWN):
        if 0 <= own < G:
            assert not np.isin(segment[0], LIMIT_ROWS).any()
            train[:, own, :] += counts_of(segment, K, W)
    # segment 1 is all its group holds of row 3: c_j == q_j for a whole row; groups 0 and 1 have never seen row 17
    assert train[3, 0].sum() == 1 and train[3, 0, W - 1] == 1 and not train[3, 1].any() and not train[17, :2].any()
    return segments, train, prior


# ------------------------------------------------------------------------------------------- sequences
def count_host(seqs_by_group, lag, alphabet):
    """{k-mer: uint32 [G, W]} of the sequences, every one padded with ``lag`` start symbols and one stop, counted on the host."""
    letters = tu.LETTERS[alphabet] + "]"
    table = {}
    for g, seqs in enumerate(seqs_by_group):
        for s in seqs:
            t = "[" * lag + s + "]"
            for p in range(lag, len(t)):
                table.setdefault(t[p - lag:p], np.zeros((len(seqs_by_group), len(letters)), np.uint32))[g, letters.index(t[p])] += 1
    return table


def string_entries(strings, lag, alphabet, table, n_groups, prior_of=None):
    """Per padded string the k-mers of ``oracle``: its contexts with the letters that follow them inside the string."""
    letters = tu.LETTERS[alphabet] + "]"
    zero = np.zeros((n_groups, len(letters)), np.uint32)
    out = []
    for s in strings:
        runs = {}
        for p in range(lag, len(s)):
            runs.setdefault(s[p - lag:p], Counter())[letters.index(s[p])] += 1
        out.append([(table.get(k, zero), None if prior_of is None else prior_of(k), q) for k, q in runs.items()])
    return out


# ------------------------------------------------------------------------------------------- the statistical case
STAT_LAGS = (1, 2)
STAT_SEEDS = {"dna": (41, 42), "prot": (43, 44)}          # the two chains of an alphabet (chosen on the CPU: test_classify_gpu.py)
STAT_VANS = np.array([1.0])


def stat_case(alphabet):
    """Two order-1 chains with different transition matrices -> ``(train, held)``: per group 200 training and 100 held-out
    sequences of 60 letters."""
    train, held = [], []
    for g, seed in enumerate(STAT_SEEDS[alphabet]):
        P = tu.chain(seed, alphabet, order=1)
        train.append(tu.sample_seqs(P, 1000 + seed, alphabet, n_seqs=200, length=60, order=1))
        held.append(tu.sample_seqs(P, 2000 + seed, alphabet, n_seqs=100, length=60, order=1))
    return train, held


def stat_oracle(alphabet, lag):
    """``(log_marg [200, 2, 1], margin [200], accuracy)`` of the held-out sequences under the vanilla model of STAT_VANS: the oracle's
    marginals, the gap between its two groups and the share of sequences whose larger one is the group that made them."""
    train, held = stat_case(alphabet)
    table = count_host(train, lag, alphabet)
    strings = ["[" * lag + s + "]" for seqs in held for s in seqs]
    want, _ = oracle(string_entries(strings, lag, alphabet, table, 2), [], STAT_VANS, len(tu.LETTERS[alphabet]) + 1, 2)
    truth = np.repeat([0, 1], 100)
    return want, np.abs(want[:, 0, 0] - want[:, 1, 0]), float((np.argmax(want[:, :, 0], 1) == truth).mean())
