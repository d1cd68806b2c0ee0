"""What the CPU and GPU tests of the k-sample Bayes factors share (bear_k_sample_f64, bear_amd.hypothesis.k_sample / agglomerate):
tests/two_sample_util.py's oracle (``_T``, ``concentrations``: the formulas of include/bear_hip.h with mpmath at 50 digits, value
and L1 mass of the terms) extended to G columns -- the group, pair and all-groups values row by row -- its SciPy twin for whole
tables, the G-column table of rows of every kind, and the six-group statistical case."""
import mpmath
import numpy as np

import two_sample_util as tu

KEYS = ("group", "pair", "all", "ar")


def pairs(G):
    """The pairs in the entry's order: (0, 1), (0, 2), ..., (G - 2, G - 1)."""
    return [(g, g2) for g in range(G) for g2 in range(g + 1, G)]


def columns(W, G):
    """``(cols uint32 [G, n, W], prior [n, W])``: columns 0 and 1 are ``a``, ``b`` of ``tu.base_rows(W)``; column g >= 2 is column
    g mod 2 with its rows rotated by 3 (g // 2), so that pairs meet rows of different kinds and 0xFFFFFFFF cells pool beyond 2^32 (to
    2^33 - 2, a row total beyond 2^37; ``limit_rows`` has the cells of all sixteen); at G >= 4 the last column is all zeros."""
    a, b, prior = tu.base_rows(W)
    cols = [np.roll((a, b)[g % 2], 3 * (g // 2), axis=0) for g in range(G)]
    if G >= 4:
        cols[-1] = np.zeros_like(a)
    return np.ascontiguousarray(np.stack(cols)), prior


def limit_rows(W, G=16):
    """``(cols [G, 3, W], prior [3, W])``: pooled counts at the entry's limits -- every cell of every column 0xFFFFFFFF (all sixteen:
    a cell of 2^36 - 16, a row total above 2^40 at width 21), one cell of every column, and every column but the first."""
    cols = np.zeros((G, 3, W), dtype=np.uint32)
    cols[:, 0, :] = tu.U32_MAX
    cols[:, 1, W - 1] = tu.U32_MAX
    cols[1:, 2, :] = tu.U32_MAX
    cols[0, 2, 0] = 1
    prior = np.random.default_rng(7).dirichlet(np.full(W, 0.5), size=3) + 1e-7
    return cols, prior / prior.sum(1, keepdims=True)


def oracle_rows(cols, prior, hs, vans):
    """Row by row, as object arrays of mpmath numbers, a dict of ``(val, mass)``: 'group' [N, M, G] = T(c_g); 'pair' [N, M, P, 2] =
    {T(c_g + c_g'), B_k} (B_k's mass: the three T it is formed from); 'all' [N, M, 2] = {T(sum_g c_g), (sum_g T(c_g)) - T(sum_g
    c_g)} (the bracket's mass: all G + 1); 'ar' [N, G] = sum_j c_gj log prior_j (zeros without prior)."""
    cols = np.asarray(cols, dtype=np.uint64)
    G, N, W = cols.shape
    M, pr = len(hs) + len(vans), pairs(G)
    shapes = {"group": (N, M, G), "pair": (N, M, len(pr), 2), "all": (N, M, 2), "ar": (N, G)}
    out = {k: (np.empty(s, dtype=object), np.empty(s, dtype=object)) for k, s in shapes.items()}
    memo = {}                       # (prior row, model, counts) -> T: the rows of a sparse table under one prior row repeat
    with mpmath.workdps(50):
        for k in range(N):
            c = [[int(x) for x in cols[g, k]] for g in range(G)]
            pooled = [sum(c[g][j] for g in range(G)) for j in range(W)]
            alphas, totals = tu.concentrations(prior[k] if prior is not None else np.zeros(W), hs, vans, W)
            pk = prior[k].tobytes() if prior is not None else b""

            def T(m, counts):
                key = (pk, m, tuple(counts))
                if key not in memo:
                    memo[key] = tu._T(alphas[m], totals[m], counts)
                return memo[key]
            for m in range(M):
                t = [T(m, c[g]) for g in range(G)]
                for g in range(G):
                    out["group"][0][k, m, g], out["group"][1][k, m, g] = t[g]
                for p, (g, g2) in enumerate(pr):
                    tp = T(m, [x + y for x, y in zip(c[g], c[g2])])
                    out["pair"][0][k, m, p] = [tp[0], (t[g][0] + t[g2][0]) - tp[0]]
                    out["pair"][1][k, m, p] = [tp[1], t[g][1] + t[g2][1] + tp[1]]
                ta = T(m, pooled)
                st, sm = t[0]
                for x in t[1:]:
                    st, sm = st + x[0], sm + x[1]
                out["all"][0][k, m] = [ta[0], st - ta[0]]
                out["all"][1][k, m] = [ta[1], sm + ta[1]]
            for g in range(G):
                terms = [c[g][j] * mpmath.log(mpmath.mpf(float(prior[k, j]))) for j in range(W) if c[g][j]] if prior is not None else []
                out["ar"][0][k, g], out["ar"][1][k, g] = mpmath.fsum(terms), mpmath.fsum(abs(x) for x in terms)
    return out


def oracle_sums(rows, idx=None):
    """The table ``base[idx]`` (``rows`` = ``oracle_rows(base...)``; None: the base itself) summed at 50 digits -> a dict of float64
    ``(val, mass)`` without the row axis."""
    n = rows["group"][0].shape[0]
    mult = np.bincount(idx, minlength=n) if idx is not None else np.ones(n, dtype=np.int64)
    with mpmath.workdps(50):
        def total(x):
            flat = x.reshape(n, -1)
            s = [mpmath.fsum(int(mult[k]) * flat[k, q] for k in range(n) if mult[k]) for q in range(flat.shape[1])]
            return np.array([float(v) for v in s]).reshape(x.shape[1:])
        return {k: (total(v[0]), total(v[1])) for k, v in rows.items()}


def scipy_sums(cols, prior, hs, vans):
    """The SciPy twin for whole tables, vectorised over the rows: float64 ``(group [M, G], pair [M, P, 2], all [M, 2], ar [G] or
    None)``."""
    from scipy.special import gammaln
    cols = np.asarray(cols, dtype=np.float64)
    G, N, W = cols.shape
    group, pair, both = [], [], []
    for m in range(len(hs) + len(vans)):
        al = prior * (1.0 / hs[m]) if m < len(hs) else np.full((N, W), float(vans[m - len(hs)]))
        A = al.sum(1)

        def T(c):
            n = c.sum(1)
            cell, nz = np.zeros(c.shape), c > 0                                # (a sparse table: the non-zero cells only)
            cell[nz] = gammaln(al[nz] + c[nz]) - gammaln(al[nz])
            cell = cell.sum(1)
            return np.where(n > 0, gammaln(A) - gammaln(A + n) + cell, 0.0)
        t = [T(cols[g]) for g in range(G)]
        group.append([x.sum() for x in t])
        tp = [T(cols[g] + cols[g2]) for g, g2 in pairs(G)]
        pair.append([[x.sum(), ((t[g] + t[g2]) - x).sum()] for x, (g, g2) in zip(tp, pairs(G))])
        ta = T(cols.sum(0))
        both.append([ta.sum(), (sum(t) - ta).sum()])
    ar = None
    if prior is not None:
        ar = np.array([np.where(c > 0, c * np.log(np.where(c > 0, prior, 1.0)), 0.0).sum() for c in cols])
    return np.array(group), np.array(pair), np.array(both), ar


def unique_rows(cols, prior):
    """``(first, inverse)`` of the distinct (columns, prior) rows of a table, as ``tu.unique_rows``: the oracle is paid per distinct row."""
    key = np.concatenate([c.astype(np.float64) for c in cols] + [prior], 1)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return first, inverse.reshape(-1)


# ------------------------------------------------------------------------------------------- the statistical case
GROUPS = ((1, 10), (2, 12), (1, 11), (2, 13), (1, 14), (2, 15))        # (chain, seed): sources alternate
PARTITION = [[0, 2, 4], [1, 3, 5]]
STAT_HS, STAT_VANS = np.array([0.05, 5.0]), np.array([1.0])             # uniform AR rows with these h, and van = 1


def stat_sequences(alphabet):
    """The six groups of 100 sequences x 120 letters: chains ``tu.chain(1)`` and ``tu.chain(2)`` at the order of ``tu.STAT_CASE``."""
    order, _ = tu.STAT_CASE[alphabet]
    chains = {c: tu.chain(c, alphabet, order) for c in (1, 2)}
    return [tu.sample_seqs(chains[c], seed, alphabet, order=order) for c, seed in GROUPS]


def count_host(seqs_by_group, lag, alphabet="dna"):
    """``tu.count_host`` for G groups -> uint32 [G, n, A + 1] over the contexts seen (sorted)."""
    letters = tu.LETTERS[alphabet] + "]"
    table = {}
    for col, seqs in enumerate(seqs_by_group):
        for s in seqs:
            t = "[" * lag + s + "]"
            for p in range(lag, len(t)):
                table.setdefault(t[p - lag:p], np.zeros((len(seqs_by_group), len(letters)), np.uint32))[col, letters.index(t[p])] += 1
    return np.ascontiguousarray(np.stack([table[k] for k in sorted(table)]).transpose(1, 0, 2))


def scipy_evaluate(model):
    """``evaluate`` of ``hypothesis.merge_loop`` on host tables uint32 [n, W] under model number ``model`` of (STAT_HS, STAT_VANS) with
    uniform AR rows; a single cluster stands beside an empty column, as in ``hypothesis.agglomerate``."""
    def evaluate(tables):
        cols = np.stack(list(tables) if len(tables) > 1 else [tables[0], np.zeros_like(tables[0])])
        G, n, W = cols.shape
        hs, vans = (STAT_HS[model:model + 1], STAT_VANS[:0]) if model < len(STAT_HS) else (STAT_HS[:0], STAT_VANS[model - len(STAT_HS):][:1])
        group, pair, _, _ = scipy_sums(cols, np.full((n, W), 1.0 / W), hs, vans)
        log_bf = np.zeros((G, G))
        for p, (g, g2) in enumerate(pairs(G)):
            log_bf[g, g2] = log_bf[g2, g] = pair[0, p, 1]
        return group[0, :len(tables)], log_bf
    return evaluate
