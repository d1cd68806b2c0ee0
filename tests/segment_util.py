"""What the CPU and GPU tests of the segmentation share (bear_score_emit_groups_f64, bear_hmm_groups_f64, bear_amd.classify.segment):
the oracles -- the emission formula and both recurrences of include/bear_hip.h evaluated with mpmath at 50 digits, a NumPy
longdouble twin of the recurrences for the cases 50 digits would take too long for, and brute force over all paths --, the
kernel cases and the statistical case.  Nothing here touches a device."""
import functools
import itertools

import mpmath
import numpy as np

import classify_util as cu
import two_sample_util as tu

RTOL = cu.RTOL                     # 1e-11 of the mass behind a value: the family's bound
MIN_GAP = 1e-6                     # a position's best and second-best max-marginal lie further apart than this in every case
NEG = float("-inf")


# ------------------------------------------------------------------------------------------- emissions
def emission_cell(c, f, letters, hs, vans):
    """The transitions of one k-mer and group to the given letters under every model -> ``(want, scale, exact)`` [3, M, letters].
    include/bear_hip.h defines the concentrations as float64 values -- ``a_j = fma(f_j, 1 / h, c_j)`` resp. ``c_j + van``, ``A`` their
    float64 sum in cell order -- so ``want`` is ``log(a_l) - log(A)`` at 50 digits OF THOSE (the fma: an exact product and sum,
    rounded once) and ``scale`` is ``|log a_l| + |log A|``; ``exact``: the same with ``a_j = f_j / h + c_j`` and ``A`` in exact
    arithmetic, which the roundings behind a_l and A -- one for 1 / h, one per a_j, one per addition -- move by at most
    ``(W + 3) * 2^-53``.  Under ``mpmath.workdps(50)``."""
    from fractions import Fraction
    W, H = len(c), len(hs)
    out = np.zeros((3, H + len(vans), len(letters)))
    for m in range(H + len(vans)):
        if m < H:
            w = Fraction(1.0 / float(hs[m]))
            a = [float(Fraction(float(f[j])) * w + int(c[j])) for j in range(W)]
            true = [mpmath.mpf(float(f[j])) / mpmath.mpf(float(hs[m])) + int(c[j]) for j in range(W)]
        else:
            a = [float(np.float64(int(c[j])) + np.float64(vans[m - H])) for j in range(W)]
            true = [mpmath.mpf(float(vans[m - H])) + int(c[j]) for j in range(W)]
        A = np.float64(0.0)
        for x in a:
            A = A + np.float64(x)
        log_A, log_true = mpmath.log(mpmath.mpf(float(A))), mpmath.log(mpmath.fsum(true))
        for k, l in enumerate(letters):
            log_a = mpmath.log(mpmath.mpf(a[l]))
            out[:, m, k] = float(log_a - log_A), float(abs(log_a) + abs(log_A)), float(mpmath.log(true[l]) - log_true)
    return out


def emission_oracle(rows, letters, train, prior, hs, vans):
    """``(want, scale, exact)`` float64 [M, n_t, G] of ``emission_cell``; zeros at a position without a transition.  Paid per
    distinct (row, group, model)."""
    K, G, W = train.shape
    M = len(hs) + len(vans)
    out = np.zeros((3, M, len(rows), G))
    live = (rows >= 0) & (rows < K) & (letters < W)
    with mpmath.workdps(50):
        for r in np.unique(rows[live]):
            at = np.flatnonzero(live & (rows == r))
            seen, inverse = np.unique(letters[at], return_inverse=True)
            for g in range(G):
                out[:, :, at, g] = emission_cell(train[r, g], prior[r], [int(l) for l in seen], hs, vans)[:, :, inverse]
    return out[0], out[1], out[2]


def input_rounding(W):
    """How far the float64 roundings behind a_l and A can move an emission from its value in exact arithmetic (``emission_cell``)."""
    return (W + 3) * 2.0 ** -53


def emit_text(K, W, n_t=4097, seed=0):
    """``(rows int32, letters uint8)`` of ``n_t`` positions in text order: 10 % hold no transition -- by a negative row (and the
    letter 0xFF), by the letter alone, by a row >= K alone."""
    rng = np.random.default_rng(900 + seed)
    rows, letters = rng.integers(0, K, n_t), rng.integers(0, W, n_t)
    u = rng.random(n_t)
    rows = np.where(u < 0.04, -1, rows)
    letters = np.where((u < 0.04) | ((u >= 0.04) & (u < 0.07)), 0xFF, letters)
    rows = np.where((u >= 0.07) & (u < 0.09), K, rows)
    rows = np.where((u >= 0.09) & (u < 0.1), 2 ** 31 - 1, rows)
    return rows.astype(np.int32), letters.astype(np.uint8)


def emit_table(K, G, W, seed=0):
    """``(train uint32 [K, G, W], prior [K, W])``: sparse Poisson counts, a k-mer no group has seen, cells at the counter's limit."""
    rng = np.random.default_rng(700 + 31 * G + W + seed)
    train = np.where(rng.random((K, G, W)) < 0.5, rng.poisson(20.0, (K, G, W)), 0).astype(np.uint32)
    train[1] = 0
    train[2, :, ::2] = 4294967295
    if K > 3:
        train[3] = 4294967295
    return train, rng.dirichlet(np.full(W, 0.5), size=K) + 1e-7


HS16 = np.array([1e-3, 0.05, 0.3, 1.0, 3.0, 30.0, 1e3, 1e6])
VANS16 = np.array([1e-3, 0.01, 0.1, 0.5, 1.0, 2.0, 10.0, 1e3])
# (K, G, BEAR models, vanilla models): the table of classify_util.kernel_case (K = 37, G = 3) under its 2 + 3 models and under 16,
# then G = 1, 16 and 256 -- the oracle is paid per (row, group, model), so the widest table has the fewest rows and models
EMIT_CASES = [("case", 3, cu.HS, cu.VANS), ("case", 3, HS16, VANS16), (37, 1, HS16, VANS16), (11, 16, cu.HS, cu.VANS),
              (5, 256, cu.HS[:1], cu.VANS[1:2])]


@functools.lru_cache(maxsize=None)
def emit_case(W, which):
    """``(rows, letters, train, prior, hs, vans, want, scale, exact)`` of EMIT_CASES[which] at width W, the oracle computed once."""
    K, G, hs, vans = EMIT_CASES[which]
    if K == "case":
        _, train, prior = cu.kernel_case(W)
    else:
        train, prior = emit_table(K, G, W)
    rows, letters = emit_text(train.shape[0], W, seed=which)
    return (rows, letters, train, prior, hs, vans) + emission_oracle(rows, letters, train, prior, hs, vans)


def string_emissions(strings, lag, alphabet, table, n_groups, hs, vans, prior_of=None):
    """``(want, scale)`` float64 [P, G, M] of the transitions of the padded strings, in order: ``emission_cell`` on the host's own
    count ``table`` ({k-mer: uint32 [G, W]}, ``classify_util.count_host``); an absent k-mer is a row of zeros."""
    letters = tu.LETTERS[alphabet] + "]"
    W, M = len(letters), len(hs) + len(vans)
    zero = np.zeros((n_groups, W), np.uint32)
    cell, want, scale = {}, [], []
    with mpmath.workdps(50):
        for s in strings:
            for p in range(lag, len(s)):
                k, l = s[p - lag:p], letters.index(s[p])
                if (k, l) not in cell:
                    c, f = table.get(k, zero), None if prior_of is None else prior_of(k)
                    cell[k, l] = np.stack([emission_cell(c[g], f, [l], hs, vans)[:, :, 0] for g in range(n_groups)], 1)      # [3, G, M]
                want.append(cell[k, l][0])
                scale.append(cell[k, l][1])
    shape = (0, n_groups, M)
    return (np.stack(want), np.stack(scale)) if want else (np.zeros(shape), np.zeros(shape))


# ------------------------------------------------------------------------------------------- the chain
def _lse(xs):
    top = max(xs)
    if top == NEG:
        return mpmath.mpf(NEG)
    return top + mpmath.log(mpmath.fsum(mpmath.exp(x - top) for x in xs if x != NEG))


def _recurrences(e, lt, ls, reduce, zero):
    """``(forward [T][S], backward [T][S])`` of one semiring, numbers of whatever kind ``e``, ``lt``, ``ls`` hold."""
    T, S = len(e), len(ls)
    fwd, bwd = [None] * T, [None] * T
    for t in range(T):
        fwd[t] = [ls[g] + e[0][g] if t == 0 else e[t][g] + reduce([fwd[t - 1][h] + lt[h][g] for h in range(S)]) for g in range(S)]
    for t in range(T - 1, -1, -1):
        bwd[t] = [zero if t == T - 1 else reduce([lt[g][h] + e[t + 1][h] + bwd[t + 1][h] for h in range(S)]) for g in range(S)]
    return fwd, bwd


def chain_mass(e, lt, ls):
    """``sum_t max_g |e_t(g)| + (T - 1) max|finite log_trans| + max|finite log_start|``: what a step's roundings are relative to."""
    e, lt, ls = np.asarray(e, dtype=np.float64), np.asarray(lt), np.asarray(ls)
    T = e.shape[0]
    return float(np.abs(e).max(1).sum() if T else 0.0) + max(T - 1, 0) * float(np.abs(lt[np.isfinite(lt)]).max()) + float(np.abs(ls[np.isfinite(ls)]).max())


def _result(fwd, bwd, dlt, eta, ls, reduce_sum, reduce_max, as_float, S):
    T = len(fwd)
    ev = reduce_sum(fwd[T - 1] if T else list(ls))
    best = reduce_max(dlt[T - 1] if T else list(ls))
    post, path, gap = np.zeros((T, S)), np.zeros(T, dtype=np.uint8), np.full(T, np.inf)
    for t in range(T):
        post[t] = [as_float(fwd[t][g] + bwd[t][g] - ev) if ev != NEG else np.nan for g in range(S)]
        mm = [as_float(dlt[t][g] + eta[t][g]) for g in range(S)]
        order = sorted(range(S), key=lambda g: (-mm[g], g))
        path[t] = order[0] if mm[order[0]] != NEG else 255
        if S > 1 and mm[order[1]] != NEG:
            gap[t] = mm[order[0]] - mm[order[1]]
    return dict(log_evidence=as_float(ev), log_best=as_float(best), log_post=post, path=path, gap=gap)


def chain_oracle(e, lt, ls):
    """One segment at 50 digits -> dict(log_evidence, log_best, log_post [T, S], path [T], gap [T]): both recurrences of
    include/bear_hip.h; ``gap``: the best less the second-best max-marginal of every step (inf where there is no second)."""
    e, lt, ls = np.asarray(e, dtype=np.float64), np.asarray(lt, dtype=np.float64), np.asarray(ls, dtype=np.float64)
    with mpmath.workdps(50):
        E = [[mpmath.mpf(float(x)) for x in row] for row in e]
        LT = [[mpmath.mpf(float(x)) for x in row] for row in lt]
        LS = [mpmath.mpf(float(x)) for x in ls]
        fwd, bwd = _recurrences(E, LT, LS, _lse, mpmath.mpf(0))
        dlt, eta = _recurrences(E, LT, LS, max, mpmath.mpf(0))
        return _result(fwd, bwd, dlt, eta, LS, _lse, max, float, len(ls))


def chain_twin(e, lt, ls):
    """``chain_oracle`` in NumPy longdouble, vectorised over the states (tests/test_segment_cpu.py holds it to the 50-digit oracle)."""
    ld = np.longdouble
    e, lt, ls = np.asarray(e, dtype=ld), np.asarray(lt, dtype=ld), np.asarray(ls, dtype=ld)
    T, S = e.shape[0], ls.size

    def lse(x, axis):
        top = x.max(axis)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = top + np.log(np.exp(x - np.expand_dims(np.where(np.isfinite(top), top, 0), axis)).sum(axis))
        return np.where(top == NEG, top, out)

    def run(reduce):
        fwd, bwd = np.zeros((T, S), dtype=ld), np.zeros((T, S), dtype=ld)
        for t in range(T):
            fwd[t] = ls + e[0] if t == 0 else e[t] + reduce(fwd[t - 1][:, None] + lt, 0)
        for t in range(T - 2, -1, -1):
            bwd[t] = reduce(lt + (e[t + 1] + bwd[t + 1])[None, :], 1)
        return fwd, bwd
    fwd, bwd = run(lse)
    dlt, eta = run(lambda x, axis: x.max(axis))
    return _result(fwd, bwd, dlt, eta, ls, lambda v: lse(np.asarray(v, dtype=ld), 0), lambda v: np.asarray(v, dtype=ld).max(), float, S)


def brute_force(e, lt, ls):
    """``chain_oracle``'s result by enumeration of all S^T paths at 50 digits (T >= 1)."""
    e, lt, ls = np.asarray(e, dtype=np.float64), np.asarray(lt, dtype=np.float64), np.asarray(ls, dtype=np.float64)
    T, S = e.shape
    with mpmath.workdps(50):
        mpf = mpmath.mpf
        score = {}
        for p in itertools.product(range(S), repeat=T):
            v = mpf(float(ls[p[0]])) + mpf(float(e[0, p[0]]))
            for t in range(1, T):
                v += mpf(float(lt[p[t - 1], p[t]])) + mpf(float(e[t, p[t]]))
            score[p] = v
        ev, best = _lse(list(score.values())), max(score.values())
        post, path = np.zeros((T, S)), np.zeros(T, dtype=np.uint8)
        for t in range(T):
            through = [[v for p, v in score.items() if p[t] == g] for g in range(S)]
            post[t] = [float(_lse(x) - ev) if ev != NEG else np.nan for x in through]
            mm = [max(x) for x in through]
            path[t] = min(g for g in range(S) if mm[g] == max(mm)) if max(mm) != NEG else 255
        winners = [p for p, v in score.items() if v == best]
        return dict(log_evidence=float(ev), log_best=float(best), log_post=post, path=path, winners=winners)


def sticky(S, switch=0.01):
    """``(log_trans, log_start)`` of ``classify.segment(switch=...)``: stay ``log(1 - switch)``, each other state ``log(switch / (S - 1))``,
    a uniform start (one state: the stay alone)."""
    lt = np.full((S, S), np.log(switch / max(S - 1, 1)))
    np.fill_diagonal(lt, np.log1p(-switch))
    return lt, np.full(S, -np.log(S))


def chains(S, seed=0):
    """{name: (log_trans, log_start)}: sticky; dense random and unnormalised; left to right -- -inf below the diagonal -- from state 0."""
    rng = np.random.default_rng(50 + S + seed)
    ltr = np.where(np.arange(S)[:, None] <= np.arange(S)[None, :], rng.normal(-1.0, 0.5, (S, S)), NEG)
    return {"sticky": sticky(S), "dense": (rng.normal(-1.5, 1.0, (S, S)), rng.normal(-1.0, 1.0, S)),
            "left_to_right": (ltr, np.where(np.arange(S) == 0, 0.0, NEG))}


def chain_lengths(S, C):
    """The segment lengths of the chain test with C = BEAR_HMM_CHUNK: empty, below, at and beyond one chunk, several chunks with a
    ragged last one; sixteen states: up to just beyond one chunk (the oracle is paid per step and pair of states)."""
    return [0, 1, C + 1] if S == 16 else [0, 1, 2, C - 1, C, C + 1, 3 * C + 17, 0]


CHAIN_SEEDS = {1: 11, 2: 12, 3: 13, 16: 16}               # chosen on the CPU: every step's gap exceeds MIN_GAP (test_segment_cpu.py)


@functools.lru_cache(maxsize=None)
def chain_case(S, name, C):
    """``(emit [n_t, S], seg [n_seg + 1], log_trans, log_start, per segment the oracle's result and its mass)``: seeded
    normal(-2, 1.5) emissions; 50 digits, the longdouble twin at sixteen states."""
    lens = chain_lengths(S, C)
    rng = np.random.default_rng(CHAIN_SEEDS[S])
    emit = rng.normal(-2.0, 1.5, (sum(lens), S))
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    lt, ls = chains(S)[name]
    solve = chain_twin if S == 16 else chain_oracle
    want = [solve(emit[a:b], lt, ls) for a, b in zip(seg[:-1], seg[1:])]
    return emit, seg, lt, ls, want, [chain_mass(emit[a:b], lt, ls) for a, b in zip(seg[:-1], seg[1:])]


# ------------------------------------------------------------------------------------------- the statistical case
STAT_SWITCH = 0.005
STAT_N, STAT_LEN = 40, 600


@functools.lru_cache(maxsize=None)
def stat_chimeras(alphabet):
    """``(seqs, truth)``: 40 chimeras of 600 letters of the two order-1 chains of ``classify_util.STAT_SEEDS`` -- A|B|A or B|A|B with
    two cut points in [60, 540] at least 60 apart, every letter drawn from the chain of its label given the letter in front of
    it -- and the label of every letter."""
    letters = tu.LETTERS[alphabet]
    A = len(letters)
    P = [tu.chain(seed, alphabet, order=1) for seed in cu.STAT_SEEDS[alphabet]]
    rng = np.random.default_rng(4000 + A)
    seqs, truth = [], []
    for i in range(STAT_N):
        while True:
            c0, c1 = sorted(int(x) for x in rng.integers(60, 541, 2))
            if c1 - c0 >= 60:
                break
        label = np.full(STAT_LEN, i % 2)
        label[c0:c1] = 1 - i % 2
        s = [int(rng.integers(0, A))]
        for t in range(1, STAT_LEN):
            s.append(int(rng.choice(A, p=P[label[t]][s[-1]])))
        seqs.append("".join(letters[x] for x in s))
        truth.append(label)
    return seqs, truth


@functools.lru_cache(maxsize=None)
def stat_oracle(alphabet, lag):
    """``(paths, gap, accuracy)`` of the chimeras under van(1) and a chain of switch probability 0.005, by the oracle alone: the
    emissions of the table counted on the host at 50 digits, the chain in longdouble.  A sequence's transitions are its letters
    and then its stop, which carries the label of the last letter."""
    train, _ = cu.stat_case(alphabet)
    table = cu.count_host(train, lag, alphabet)
    letters = tu.LETTERS[alphabet] + "]"
    W = len(letters)
    seqs, truth = stat_chimeras(alphabet)
    lt, ls = sticky(2, STAT_SWITCH)
    cell = {}
    paths, gaps, hits, total = [], [], 0, 0
    zero = np.zeros((2, W), np.uint32)
    with mpmath.workdps(50):
        for s, label in zip(seqs, truth):
            t = "[" * lag + s + "]"
            e = np.zeros((len(t) - lag, 2))
            for p in range(lag, len(t)):
                k, j = t[p - lag:p], letters.index(t[p])
                if (k, j) not in cell:
                    c = table.get(k, zero)
                    cell[k, j] = [float(mpmath.log(mpmath.mpf(int(c[g, j]) + 1) / mpmath.mpf(int(c[g].astype(np.int64).sum()) + W))) for g in range(2)]
                e[p - lag] = cell[k, j]
            res = chain_twin(e, lt, ls)
            want = np.concatenate([label, label[-1:]])
            paths.append(res["path"])
            gaps.append(res["gap"].min())
            hits, total = hits + int((res["path"] == want).sum()), total + want.size
    return paths, float(min(gaps)), hits / total
