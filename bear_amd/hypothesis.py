"""Hypothesis tests under BMM and BEAR models, on the device: are two samples of sequences from one distribution, and is the
parametric AR model enough for a sample or does the data favour the nonparametric BEAR model around it?  And among G samples
(``k_sample``, one pass over the table: ``bear_k_sample_f64``, kernels_ksample.h): which differ from which, are all of them one
distribution, and which belong together (``agglomerate``: greedy Bayesian clustering of the samples).

Both are sums over the rows of a count table whose two samples are two columns (``bear_two_sample_f64``, kernels_twosample.h).
Per context ``k`` and model the log marginal of the transitions as sequences is

    T(c) = lgamma(A) - lgamma(A + n) + sum_j [lgamma(alpha_j + c_j) - lgamma(alpha_j)]

with ``alpha_j = ar_func(k)_j / h`` (BEAR) or ``van`` (vanilla BMM).  The two-sample log Bayes factor of "two distributions" over
"one" is ``sum_k [T(a_k) + T(b_k) - T(a_k + b_k)]`` (positive favours different), formed per row: a context seen in one sample only
adds exactly zero.  The goodness-of-fit log Bayes factor of BEAR(h) over its embedded AR model is ``sum_k T(a_k) - sum_k sum_j a_j
log ar_func(k)_j``.  Nothing here computes: the rows of the AR function come from its kernels, the sums from one launch per piece
of the table and at most four models."""
import numpy as np
import torch

from . import core, dataloader, kernels


class TwoSampleResult:
    """``models``: a label per model, the BEAR models (one per h) first, then the vanilla ones; ``log_bf`` float64 [n_models]: the
    two-sample log Bayes factor, positive favours two distributions; ``log_marg`` float64 [n_models, 3]: the log marginals of
    sample a, sample b and the pooled sample; ``log_ar`` float64 [2] or None: the AR model's log-likelihood of a and b;
    ``per_kmer``: CUDA float64 [N, n_models], each context's term of ``log_bf`` (which contexts drive a difference), or None."""

    def __init__(self, models, n_h, sums, log_ar, per_kmer):
        self.models = list(models)
        self.n_h = int(n_h)
        self.log_marg = np.ascontiguousarray(sums[:, :3])
        self.log_bf = np.ascontiguousarray(sums[:, 3])
        self.log_ar = log_ar
        self.per_kmer = per_kmer

    def gof_log_bf(self):
        """float64 [n_h, 2]: the log Bayes factor of every BEAR model over its embedded AR model, for sample a and sample b
        (positive: the data favour the nonparametric model)."""
        if self.log_ar is None:
            return np.zeros((0, 2))
        return self.log_marg[:self.n_h, :2] - self.log_ar[None, :]

    def __repr__(self):
        return "TwoSampleResult(" + ", ".join(f"{m}: {v:.6g}" for m, v in zip(self.models, self.log_bf)) + ")"


def _check_model(bear_path, ar_func, h, vans):
    """The refusals that need neither the table nor a device -> ``(hs or None, vans)`` as float64 vectors."""
    if bear_path is not None and (ar_func is not None or h is not None):
        raise ValueError("give either bear_path (its AR function and fitted h) or ar_func with h, not both")
    if (ar_func is None) != (h is None):
        raise ValueError("ar_func and h come together: the BEAR models are ar_func's rows over every h")
    vs = np.atleast_1d(np.asarray(vans, dtype=np.float64)).reshape(-1)
    hs = None if h is None else np.atleast_1d(np.asarray(h, dtype=np.float64)).reshape(-1)
    if bear_path is None and (hs is None or not hs.size) and not vs.size:
        raise ValueError("no model: give bear_path, ar_func with h, or vans")
    for name, v in (("h", hs), ("vans", vs)):
        if v is not None and not (np.all(v > 0) and np.all(np.isfinite(v))):
            raise ValueError(f"every value of {name} must be > 0 and finite")
    n = (1 if bear_path is not None else (0 if hs is None else hs.size)) + vs.size
    if n > kernels.TWO_SAMPLE_MAX_MODELS:
        raise ValueError(f"{n} models: one test takes at most {kernels.TWO_SAMPLE_MAX_MODELS}")
    return hs, vs


def _check_whole_table(data):
    if not isinstance(data, dataloader.CountDataset):
        raise ValueError("data must be a CountDataset or a DeviceCountDataset")
    if isinstance(data, dataloader.KmerDealtDataset) or data.shard is not None:
        raise ValueError("a sharded or k-mer-dealt table holds part of the rows: the test sums over the whole table (load it unsharded)")


def _check_table(data, col_a, col_b):
    _check_whole_table(data)
    if int(col_a) == int(col_b):
        raise ValueError(f"col_a and col_b are both {col_a}: a sample is not tested against itself")


def _check_col_range(data, cols):
    for c in cols:
        if not 0 <= int(c) < data.num_ds:
            raise ValueError(f"column {c}: the table has {data.num_ds}")


def _resolve_models(data, bear_path, ar_func, hs, vs, late_cols=()):
    """Behind ``_check_model`` and the table's refusals: the AR function and fitted h of ``bear_path``, held to the table's lag and
    alphabet; no h: none; the width the kernels take -> ``(ar_func, hs, the models' labels)``.  ``late_cols``: the columns that
    ``two_sample`` holds to the table's range behind the model load (``k_sample`` has done so in front of it)."""
    if bear_path is not None:
        from . import get_var_probs
        lag, alphabet, h_fit, ar_func, _ = get_var_probs.load_bear(bear_path)
        if lag != data.lag or alphabet != data.alphabet:
            raise ValueError(f"{bear_path}: a lag-{lag} model of {alphabet!r}, the table has lag {data.lag} of {data.alphabet!r}")
        hs = np.array([h_fit], dtype=np.float64)
    if hs is None:
        hs = np.zeros(0)
    _check_col_range(data, late_cols)
    if data.width not in kernels.WIDE_WIDTHS:
        raise ValueError(f"rows of width {data.width}; the kernels take {kernels.WIDE_WIDTHS}")
    return ar_func, hs, [f"bear(h={v:g})" for v in hs] + [f"van({v:g})" for v in vs]


def _device_of(data, device):
    """``device``, or where a ``DeviceCountDataset`` lives, or "cuda"."""
    on_device = isinstance(data, dataloader.DeviceCountDataset)
    return torch.device(device if device is not None else (data.counts_dev.device if on_device else "cuda"))


def _pieces(data, ar_func, device):
    """The table in pieces of ``data.batch_size`` rows -> ``(lo, hi, prior)`` per piece, ``prior`` the AR function's float64 rows
    [hi - lo, W] of the piece's k-mers on ``device`` (None without ``ar_func``): one piece's rows are resident at a time."""
    for lo, hi in data.batch_bounds():
        prior = None
        if ar_func is not None:
            if isinstance(data, dataloader.DeviceCountDataset):
                codes = kernels.encode_kmers(data.kmers_dev[lo:hi].contiguous(), data.alphabet)
            else:
                codes = torch.from_numpy(core.encode_kmers(data.kmers[lo:hi], data.alphabet)).to(device)
            with torch.no_grad():
                prior = ar_func(codes).to(torch.float64).expand(hi - lo, data.width).contiguous()
        yield lo, hi, prior


def _sum_pieces(data, ar_func, device, shapes, n_ar, n_models, per_kmer, piece):
    """``piece(lo, hi, prior)`` -> ``(*outs, out_ar, row_terms)`` on every piece of the table, the outputs (of ``shapes``; ``out_ar``
    [n_ar]) added in piece order, the row terms collected -> ``(the sums on the host, log_ar on the host or None, per_kmer [N,
    n_models] on the device or None)``.  Under the caller's device context."""
    sums = [torch.zeros(shape, dtype=torch.float64, device=device) for shape in shapes]
    log_ar = torch.zeros(n_ar, dtype=torch.float64, device=device) if ar_func is not None else None
    rows = []
    for lo, hi, prior in _pieces(data, ar_func, device):
        *out, out_ar, terms = piece(lo, hi, prior)
        sums = [s + o for s, o in zip(sums, out)]
        if out_ar is not None:
            log_ar = log_ar + out_ar
        if terms is not None:
            rows.append(terms)
        del prior
    terms = None
    if per_kmer:
        terms = torch.cat(rows, 0) if rows else torch.zeros((0, n_models), dtype=torch.float64, device=device)
    return [s.cpu().numpy() for s in sums], None if log_ar is None else log_ar.cpu().numpy(), terms


def two_sample(data, col_a, col_b, *, bear_path=None, ar_func=None, h=None, vans=(), per_kmer=False, device=None):
    """The two-sample test of columns ``col_a`` and ``col_b`` of the count table ``data`` (a ``CountDataset``, whose columns are
    uploaded with ``device_column``, or a ``DeviceCountDataset``, used in place) -> ``TwoSampleResult``.

    Models: ``bear_path`` (a trained folder: ``get_var_probs.load_bear``'s AR function and fitted h) or ``ar_func`` (codes
    [n, lag] -> rows [n, W]) with ``h`` (one value or several), and / or vanilla pseudo-counts ``vans``.  With an AR function the
    result also carries ``log_ar`` and ``gof_log_bf()``.  The rows go through in pieces of ``data.batch_size``: only one piece's AR
    rows are resident at a time, and the pieces' sums are added in piece order.  ``ValueError``, before a device is touched: a
    sharded or k-mer-dealt table, equal columns, no model, an h or van that is not > 0."""
    hs, vs = _check_model(bear_path, ar_func, h, vans)
    _check_table(data, col_a, col_b)
    ar_func, hs, models = _resolve_models(data, bear_path, ar_func, hs, vs, late_cols=(col_a, col_b))
    device = _device_of(data, device)
    with torch.cuda.device(device):
        a, b = data.device_column(int(col_a), device), data.device_column(int(col_b), device)
        (sums,), log_ar, terms = _sum_pieces(
            data, ar_func, device, [(len(models), 4)], 2, len(models), per_kmer,
            lambda lo, hi, prior: kernels.two_sample(a[lo:hi], b[lo:hi], prior, hs, vs, want_ar=ar_func is not None, want_rows=per_kmer))
        return TwoSampleResult(models, hs.size, sums, log_ar, terms)


def two_sample_from_sequences(seqs_a, seqs_b, lags, alphabet_name="dna", reverse=False, batch_size=1 << 30, **model):
    """The test of two lists of sequences (str), one result per lag of ``lags``: the sequences are encoded with groups 0 and 1
    (``summarize.encode_sequences``), counted per lag on the device (``summarize.count_transitions`` with two groups) and tested
    as columns 0 and 1 -- the table never leaves the device.  ``model``: the keywords of ``two_sample`` (an ``ar_func`` must take
    the codes of every lag asked for; ``bear_path`` fits one lag).  ``alphabet_name``: 'dna' or 'prot' (no ``reverse`` there)."""
    from . import summarize
    _check_model(model.get("bear_path"), model.get("ar_func"), model.get("h"), model.get("vans", ()))
    seqs_a, seqs_b = list(seqs_a), list(seqs_b)
    text, group = summarize.encode_sequences(seqs_a + seqs_b, [0] * len(seqs_a) + [1] * len(seqs_b), reverse, alphabet_name)
    device = torch.device(model.get("device") or "cuda")
    t, g = torch.from_numpy(text).to(device), torch.from_numpy(group).to(device)
    results = []
    for lag in lags:
        kmers, counts = summarize.count_transitions(t, g, int(lag), 2, on_device=True, alphabet=alphabet_name)
        data = dataloader.DeviceCountDataset(kmers, counts, alphabet_name, batch_size)
        results.append(two_sample(data, 0, 1, **model))
    return results


# ------------------------------------------------------------------------------------------- G samples
class KSampleResult:
    """Of G samples (columns) and M models (``models``: the BEAR models, one per h, first, then the vanilla ones), float64:
    ``log_marg`` [M, G] the log marginal of every sample; ``log_marg_pair`` [M, G, G] that of every pooled pair (symmetric, the
    diagonal is ``log_marg``); ``log_bf`` [M, G, G] the two-sample log Bayes factor of every pair, positive favours two
    distributions (symmetric, the diagonal exactly 0); ``log_marg_all`` [M] the log marginal of all samples pooled and ``log_bf_all``
    [M] the log Bayes factor of "G distributions" over "one"; ``log_ar`` [G] or None: the AR model's log-likelihood of every sample;
    ``per_kmer``: CUDA float64 [N, M], each context's term of ``log_bf_all``, or None."""

    def __init__(self, models, n_h, out_group, out_pair, out_all, log_ar, per_kmer):
        self.models = list(models)
        self.n_h = int(n_h)
        self.log_marg = np.ascontiguousarray(out_group)
        M, G = self.log_marg.shape
        self.log_marg_pair, self.log_bf = np.zeros((M, G, G)), np.zeros((M, G, G))
        upper = np.triu_indices(G, 1)                       # the entry's pair order: (0, 1), (0, 2), ..., (G - 2, G - 1)
        for full, k in ((self.log_marg_pair, 0), (self.log_bf, 1)):
            full[:, upper[0], upper[1]] = out_pair[:, :, k]
            full[:, upper[1], upper[0]] = out_pair[:, :, k]
        self.log_marg_pair[:, np.arange(G), np.arange(G)] = self.log_marg
        self.log_marg_all = np.ascontiguousarray(out_all[:, 0])
        self.log_bf_all = np.ascontiguousarray(out_all[:, 1])
        self.log_ar = log_ar
        self.per_kmer = per_kmer

    def gof_log_bf(self):
        """float64 [n_h, G]: the log Bayes factor of every BEAR model over its embedded AR model, sample by sample."""
        if self.log_ar is None:
            return np.zeros((0, self.log_marg.shape[1]))
        return self.log_marg[:self.n_h] - self.log_ar[None, :]

    def __repr__(self):
        return "KSampleResult(" + ", ".join(f"{m}: {v:.6g}" for m, v in zip(self.models, self.log_bf_all)) + ")"


def _check_cols(data, cols):
    """The refusals of the chosen columns -> the list of them (None: every column of the table)."""
    _check_whole_table(data)
    cols = list(range(data.num_ds)) if cols is None else [int(c) for c in cols]
    if len(cols) < 2:
        raise ValueError(f"{len(cols)} columns: a test among samples takes at least 2")
    if len(cols) > kernels.K_SAMPLE_MAX_GROUPS:
        raise ValueError(f"{len(cols)} columns: one call takes at most {kernels.K_SAMPLE_MAX_GROUPS}")
    if len(set(cols)) != len(cols):
        raise ValueError(f"columns {cols}: a column is repeated, and a sample is not tested against itself")
    _check_col_range(data, cols)
    return cols


def k_sample(data, cols=None, *, bear_path=None, ar_func=None, h=None, vans=(), per_kmer=False, device=None):
    """The test among the columns ``cols`` (2..16 distinct indices, in any order; None: all) of the count table ``data`` ->
    ``KSampleResult``: every sample's marginal, every pair's two-sample Bayes factor and the all-samples one, from ONE pass over
    the table per piece of ``data.batch_size`` rows (``two_sample`` on every pair reads each column and evaluates each sample's
    terms G - 1 times).  A ``DeviceCountDataset`` is used in place, a ``CountDataset`` uploads the chosen columns.  The models are
    ``two_sample``'s.  ``ValueError``, before a device is touched: what ``two_sample`` refuses, fewer than 2 or more than 16
    columns, a repeated column.  Not offered: more than 16 samples a call, sharded or k-mer-dealt tables; the sums are not the
    bits of ``two_sample`` on a pair, nor the same bits under another order of the columns (the reduction orders differ)."""
    hs, vs = _check_model(bear_path, ar_func, h, vans)
    cols = _check_cols(data, cols)
    ar_func, hs, models = _resolve_models(data, bear_path, ar_func, hs, vs)
    device = _device_of(data, device)
    n_models, G = len(models), len(cols)
    with torch.cuda.device(device):
        if isinstance(data, dataloader.DeviceCountDataset):
            table, use = data.counts_dev.to(device), cols
        else:
            table, use = torch.stack([data.device_column(c, device) for c in cols]), list(range(G))
        sums, log_ar, terms = _sum_pieces(
            data, ar_func, device, [(n_models, G), (n_models, G * (G - 1) // 2, 2), (n_models, 2)], G, n_models, per_kmer,
            lambda lo, hi, prior: kernels.k_sample(table[:, lo:hi], use, prior, hs, vs, want_ar=ar_func is not None, want_rows=per_kmer))
        return KSampleResult(models, hs.size, *sums, log_ar, terms)


def k_sample_from_sequences(seqs_by_group, lags, alphabet_name="dna", reverse=False, batch_size=1 << 30, **model):
    """``k_sample`` of G lists of sequences (str), one result per lag of ``lags``: encoded with groups 0 .. G - 1, counted per lag on
    the device with G groups and tested as columns 0 .. G - 1, as ``two_sample_from_sequences`` does with two."""
    from . import summarize
    _check_model(model.get("bear_path"), model.get("ar_func"), model.get("h"), model.get("vans", ()))
    groups = [list(s) for s in seqs_by_group]
    if not 2 <= len(groups) <= kernels.K_SAMPLE_MAX_GROUPS:
        raise ValueError(f"{len(groups)} groups of sequences: one call takes 2 to at most {kernels.K_SAMPLE_MAX_GROUPS}")
    text, group = summarize.encode_sequences([s for seqs in groups for s in seqs], [g for g, seqs in enumerate(groups) for _ in seqs],
                                             reverse, alphabet_name)
    device = torch.device(model.get("device") or "cuda")
    t, g = torch.from_numpy(text).to(device), torch.from_numpy(group).to(device)
    results = []
    for lag in lags:
        kmers, counts = summarize.count_transitions(t, g, int(lag), len(groups), on_device=True, alphabet=alphabet_name)
        results.append(k_sample(dataloader.DeviceCountDataset(kmers, counts, alphabet_name, batch_size), None, **model))
    return results


class Agglomeration:
    """``merges``: a list of ``(members_a, members_b, log_bf)``, the column indices of the two clusters of every step and the log
    Bayes factor they were merged at (negative); ``partition``: the clusters left, sorted lists of column indices; ``log_evidence``
    float64 [steps + 1]: the sum of the clusters' log marginals at the start and after every step -- a step gains -log_bf."""

    def __init__(self, merges, partition, log_evidence):
        self.merges, self.partition, self.log_evidence = merges, partition, np.asarray(log_evidence, dtype=np.float64)

    def __repr__(self):
        return f"Agglomeration({self.partition}, log evidence {self.log_evidence[-1]:.6g} after {len(self.merges)} merges)"


def merge_loop(tables, names, evaluate, pool):
    """Greedy evidence ascent over clusters of samples -> ``Agglomeration``.  ``tables``: one count table per sample, ``names`` their
    column indices; ``evaluate(tables)`` -> ``(log_marg [K], log_bf [K, K])`` of a list of K >= 1 cluster tables; ``pool(a, b)`` ->
    the table of two clusters merged.  Every step evaluates the current clusters once and merges the pair with the smallest
    ``log_bf`` (ties: the lower (g, g')); it stops when no pair is below 0 or one cluster is left."""
    tables, members = list(tables), [[int(c)] for c in names]
    log_marg, log_bf = evaluate(tables)
    merges, evidence = [], [float(np.sum(log_marg))]
    while len(tables) > 1:
        best = None
        for g in range(len(tables)):
            for g2 in range(g + 1, len(tables)):
                if best is None or log_bf[g, g2] < log_bf[best]:
                    best = (g, g2)
        if not log_bf[best] < 0:
            break
        g, g2 = best
        merges.append((sorted(members[g]), sorted(members[g2]), float(log_bf[best])))
        tables[g] = pool(tables[g], tables[g2])
        members[g] = members[g] + members[g2]
        del tables[g2], members[g2]
        log_marg, log_bf = evaluate(tables)
        evidence.append(float(np.sum(log_marg)))
    return Agglomeration(merges, sorted(sorted(m) for m in members), evidence)


def _pool_columns(a, b):
    """Two count columns (uint32 in int32 storage, on the device) pooled: int64 sums, stored back as uint32."""
    s = (a.to(torch.int64) & 0xFFFFFFFF) + (b.to(torch.int64) & 0xFFFFFFFF)
    if bool((s > 0xFFFFFFFF).any()):
        raise ValueError("a pooled cell reaches 2^32: the merged cluster does not fit a count table's 32-bit cells")
    return torch.where(s > 0x7FFFFFFF, s - (1 << 32), s).to(torch.int32)


def agglomerate(data, cols=None, *, model=0, device=None, **model_kwargs):
    """Greedy Bayesian clustering of the samples ``cols`` (None: all) of the count table ``data`` -> ``Agglomeration``: every step
    is one ``k_sample`` call on the current clusters and merges the pair with the smallest log Bayes factor under model number
    ``model`` (of ``k_sample``'s ``models``), until no pair is below 0 or one cluster is left.  A merged cluster's column is the
    int64 sum of its two on the device, stored back as uint32: a pooled cell of 2^32 or more is a ``ValueError``.
    ``model_kwargs``: the model keywords of ``k_sample``.  At most 16 samples."""
    hs, vs = _check_model(model_kwargs.get("bear_path"), model_kwargs.get("ar_func"), model_kwargs.get("h"), model_kwargs.get("vans", ()))
    cols = _check_cols(data, cols)
    n_models = (1 if model_kwargs.get("bear_path") is not None else (0 if hs is None else hs.size)) + vs.size
    if not 0 <= int(model) < n_models:
        raise ValueError(f"model {model}: the test has {n_models}")
    if "per_kmer" in model_kwargs:
        raise ValueError("agglomerate returns no per-context terms (per_kmer belongs to k_sample)")
    device = _device_of(data, device)
    with torch.cuda.device(device):
        kmers = data.kmers_dev.to(device) if isinstance(data, dataloader.DeviceCountDataset) else torch.from_numpy(np.ascontiguousarray(data.kmers)).to(device)
        columns = [data.device_column(c, device) for c in cols]

        def evaluate(tables):
            both = list(tables) if len(tables) > 1 else [tables[0], torch.zeros_like(tables[0])]    # one cluster: beside an empty column
            res = k_sample(dataloader.DeviceCountDataset(kmers, torch.stack(both), data.alphabet, data.batch_size), None, device=device, **model_kwargs)
            return res.log_marg[int(model), :len(tables)], res.log_bf[int(model)]
        return merge_loop(columns, cols, evaluate, _pool_columns)
