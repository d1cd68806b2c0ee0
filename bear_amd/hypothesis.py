"""Hypothesis tests under BMM and BEAR models, on the device: are two samples of sequences from one distribution, and is the
parametric AR model enough for a sample or does the data favour the nonparametric BEAR model around it?

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


def _check_table(data, col_a, col_b):
    if not isinstance(data, dataloader.CountDataset):
        raise ValueError("data must be a CountDataset or a DeviceCountDataset")
    if isinstance(data, dataloader.KmerDealtDataset) or data.shard is not None:
        raise ValueError("a sharded or k-mer-dealt table holds part of the rows: the test sums over the whole table (load it unsharded)")
    if int(col_a) == int(col_b):
        raise ValueError(f"col_a and col_b are both {col_a}: a sample is not tested against itself")


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
    if bear_path is not None:
        from . import get_var_probs
        lag, alphabet, h_fit, ar_func, _ = get_var_probs.load_bear(bear_path)
        if lag != data.lag or alphabet != data.alphabet:
            raise ValueError(f"{bear_path}: a lag-{lag} model of {alphabet!r}, the table has lag {data.lag} of {data.alphabet!r}")
        hs = np.array([h_fit], dtype=np.float64)
    if hs is None:
        hs = np.zeros(0)
    for c in (col_a, col_b):
        if not 0 <= int(c) < data.num_ds:
            raise ValueError(f"column {c}: the table has {data.num_ds}")
    width = data.width
    if width not in kernels.WIDE_WIDTHS:
        raise ValueError(f"rows of width {width}; the kernels take {kernels.WIDE_WIDTHS}")
    on_device = isinstance(data, dataloader.DeviceCountDataset)
    device = torch.device(device if device is not None else (data.counts_dev.device if on_device else "cuda"))
    n_models = hs.size + vs.size
    models = [f"bear(h={v:g})" for v in hs] + [f"van({v:g})" for v in vs]
    with torch.cuda.device(device):
        a, b = data.device_column(int(col_a), device), data.device_column(int(col_b), device)
        sums = torch.zeros((n_models, 4), dtype=torch.float64, device=device)
        log_ar = torch.zeros(2, dtype=torch.float64, device=device) if ar_func is not None else None
        rows = []
        for lo, hi in data.batch_bounds():
            prior = None
            if ar_func is not None:
                if on_device:
                    codes = kernels.encode_kmers(data.kmers_dev[lo:hi].contiguous(), data.alphabet)
                else:
                    codes = torch.from_numpy(core.encode_kmers(data.kmers[lo:hi], data.alphabet)).to(device)
                with torch.no_grad():
                    prior = ar_func(codes).to(torch.float64).expand(hi - lo, width).contiguous()
            out, out_ar, terms = kernels.two_sample(a[lo:hi], b[lo:hi], prior, hs, vs, want_ar=ar_func is not None, want_rows=per_kmer)
            sums = sums + out
            if out_ar is not None:
                log_ar = log_ar + out_ar
            if terms is not None:
                rows.append(terms)
            del prior
        terms = None
        if per_kmer:
            terms = torch.cat(rows, 0) if rows else torch.zeros((0, n_models), dtype=torch.float64, device=device)
        return TwoSampleResult(models, hs.size, sums.cpu().numpy(), None if log_ar is None else log_ar.cpu().numpy(), terms)


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
