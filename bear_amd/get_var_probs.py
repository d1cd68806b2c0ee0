"""Posterior predictive scores of variants and sequences: host mirror of ``bear_model/get_var_probs.py``.

Same functions and argument meaning as the reference: ``get_pdf`` (get_var_probs.py:91-194),
``get_bear_probs`` (:330-452), ``get_bear_probs_seqs`` (:498-631), ``parse_var`` (:323-328), ``load_bear``
(:58-82), ``load_ds`` (:36-56).  The numerical part of ``get_pdf`` -- concentrations of every model, the
log-Gamma draws of ``log_gamma.log_gamma`` and their normalisation, or the MAP table -- is one launch of
``bear_logdir_sample_f64`` over the batch of k-mers (``kernels_sample.h``); the exact marginal term
(``get_marg``) is one launch of ``bear_eval_f64``.  The protein alphabet (rows of 21: 20 letters + stop) takes their
width-taking twins, ``bear_logdir_sample_wide_f64`` and ``bear_eval_wide_f64``.  The k+1-mer bookkeeping stays on the host as in the
reference (string windows, a lookup table indexed by k+1-mer) -- unless the counts come from a ``DeviceCounter``: then
``get_bear_probs`` / ``get_bear_probs_seqs`` run on the device from the queries' symbols to the scores (``kernels_score.h``; the
exact marginal when ``marg_on_device=True`` asks for it, ``kernels_marg.h``; with ``moments=True`` the exact mean and variance of
the scores instead of samples of them, ``kernels_moments.h``).

Differences a user can see: draws come from a counter-based stream (``seed`` argument; ``None`` takes a fresh
seed from numpy's global generator) instead of numpy's Mersenne twister, and the KMC database look-up
(``make_kmc_genome_counter``, :213-290, external ``py_kmc_api``) is replaced by ``make_sequence_counter``: the same counts
from the sequence files themselves, counted on the device and passed as ``counter=``.
"""
import configparser
import json
import math
import os
import pickle

import numpy as np
import torch

from . import ar_funcs, bear_net, bear_ref, core, dataloader, kernels
from .log_gamma import _next_seed

epsilon = core.epsilon


def cross_str_arrays(array1, array2, exch="X"):
    """get_var_probs.py:23-34: every string of array1 followed by every string of array2, array1-major."""
    a1 = np.asarray(array1).astype(str)
    a2 = np.asarray(array2).astype(str)
    return np.char.add(a1[:, None], a2[None, :]).reshape(-1)


def load_ds(files_path, start_token, kmer_batch_size, sparse, alphabet, num_ds, dtype=torch.float64):
    """get_var_probs.py:36-56."""
    files = sorted(os.path.join(files_path, f) for f in os.listdir(files_path) if f.startswith(start_token))
    load = dataloader.sparse_dataloader if sparse else dataloader.dataloader
    parts = [load(f, alphabet, kmer_batch_size, num_ds, cache=False, dtype=dtype) for f in files]
    return parts[0] if len(parts) == 1 else dataloader.concatenate(parts)


def load_bear(path):
    """get_var_probs.py:58-82: a trained model folder (config.cfg + results.pickle) ->
    ``(lag, alphabet, h, ar_func, data)``; ``ar_func`` is the reference's ``softmax(ar_func(.)) + epsilon``
    wrapper (:79-81)."""
    config = configparser.ConfigParser()
    config.read(os.path.join(path, "config.cfg"))
    dtype = getattr(torch, config["general"]["precision"])
    lag = int(config["hyperp"]["lag"])
    alphabet = config["data"]["alphabet"]
    alphabet_size = len(core.alphabets_tf[alphabet]) - 1
    make_ar_func = getattr(ar_funcs, "make_ar_func_" + config["model"]["ar_func_name"])
    af_kwargs = json.loads(config["model"]["af_kwargs"])
    with open(os.path.join(path, "results.pickle"), "rb") as fr:
        params_restart = pickle.load(fr)["params"]
    device = torch.device("cuda", torch.cuda.current_device())
    params, h_signed, ar_func = bear_net.change_scope_params(lag, alphabet_size, make_ar_func, af_kwargs, params_restart,
                                                             dtype=dtype, device=device)
    h = float(np.exp(h_signed.item()))
    data = _load_data(config)

    def ar_func_tf(kmers):
        with torch.no_grad():
            return torch.softmax(ar_func(kmers), dim=-1) + epsilon
    return lag, alphabet, h, ar_func_tf, data


def _load_data(config):
    """The count table a model folder's config names, as ``load_bear`` loads it."""
    alphabet, files_path = config["data"]["alphabet"], config["data"]["files_path"]
    if files_path == "TEST":
        return dataloader.dataloader(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "ysd1_lag_5_file_0_preshuf.tsv"),
                                     alphabet, int(float(config["train"]["batch_size"])) or 1, int(config["data"]["num_ds"]))
    return load_ds(files_path, config["data"]["start_token"], int(float(config["train"]["batch_size"])),
                   config["data"]["sparse"] == "True", alphabet, int(config["data"]["num_ds"]))


class RefModel:
    """A model trained by ``bear_ref`` as scoring and generation take it: ``lag``, ``alphabet`` (a name of ``core.alphabets_en``),
    ``h``, ``tau`` and ``net_weight`` (host floats: the exponentials of the trained ``h_signed``, ``tau_signed`` and
    ``net_weight_signed``) and ``net_func``: None for the stop net function, else the callable from ``core.encode_kmers`` codes to
    the net function's rows ``g`` (the linear one carries ``linear_mat`` / ``fused``).  The AR function's row of a k-mer is
    ``(net_weight g + jukes_cantor(reference row, tau)) / (net_weight + 1) + epsilon`` (``kernels.ref_prior_rows``): a function of
    the k-mer's reference counts, which ``ref_counter=`` supplies."""

    def __init__(self, lag, alphabet, h, tau, net_weight, net_func=None):
        self.lag, self.alphabet = int(lag), str(alphabet)
        self.h, self.tau, self.net_weight = float(h), float(tau), float(net_weight)
        self.net_func = net_func
        if self.alphabet not in core.alphabets_en:
            raise ValueError(f"alphabet {alphabet!r} is none of {sorted(core.alphabets_en)}")
        if not (self.lag >= 1 and all(np.isfinite(v) and v > 0 for v in (self.h, self.tau, self.net_weight))):
            raise ValueError("RefModel: lag >= 1, and h, tau and net_weight finite and > 0")

    def net_rows(self, codes):
        """The net function's rows float64 [n, W] of k-mers given as codes int8 [n, lag]; None for the stop net function."""
        if self.net_func is None:
            return None
        with torch.no_grad():
            return self.net_func(codes).to(torch.float64).expand(codes.shape[0], len(core.alphabets_en[self.alphabet])).contiguous()


def load_bear_ref(path):
    """A folder written by ``models/train_bear_ref.py`` (config.cfg + results.pickle) -> ``(ref_model, data, ds_loc, ds_loc_ref)``:
    the ``RefModel``, the count table as ``load_bear`` loads it, and its training and reference columns
    (``DeviceCounter.from_dataset(data, ds_loc)`` and ``(data, ds_loc_ref)`` are the ``counter=`` and ``ref_counter=`` of the model).
    ``ValueError`` for a folder trained by ``bear_net``: its parameter list has no ``tau_signed`` / ``net_weight_signed``."""
    config = configparser.ConfigParser()
    config.read(os.path.join(path, "config.cfg"))
    dtype = getattr(torch, config["general"]["precision"])
    lag = int(config["hyperp"]["lag"])
    alphabet = config["data"]["alphabet"]
    alphabet_size = len(core.alphabets_tf[alphabet]) - 1
    make_net_func = getattr(ar_funcs, "make_ar_func_" + config["model"]["ar_func_name"])
    af_kwargs = json.loads(config["model"]["af_kwargs"])
    with open(os.path.join(path, "results.pickle"), "rb") as fr:
        params_restart = pickle.load(fr)["params"]
    if "reference_column" not in config["data"]:
        raise ValueError(f"{path}: config.cfg names no [data] reference_column: not a folder of train_bear_ref.py")
    device = torch.device("cuda", torch.cuda.current_device())
    if len(params_restart) < 3 or any(np.ndim(p) != 0 for p in params_restart[:3]):
        raise ValueError(f"{path}: the saved parameters do not start with the scalars h_signed, tau_signed, net_weight_signed of a "
                         "bear_ref model: the folder was trained by bear_net (load_bear reads it)")
    params, h_signed, ar_func = bear_ref.change_scope_params(lag, alphabet_size, make_net_func, af_kwargs, params_restart,
                                                             dtype=dtype, device=device)
    model = RefModel(lag, alphabet, math.exp(h_signed.item()), math.exp(ar_func.tau_signed.item()), math.exp(ar_func.net_weight_signed.item()),
                     None if ar_func.net_is_stop else ar_func.net_func)
    return model, _load_data(config), int(config["data"]["train_column"]), int(config["data"]["reference_column"])


class _RefRows:
    """What stands in the place of ``ar_func`` on the device path when a reference model scores: ``_prior_rows`` takes the rows from
    ``kernels.ref_prior_rows`` instead of calling it."""

    def __init__(self, model, ref_counter):
        self.model, self.ref_counter = model, ref_counter

    def rows(self, counter, kmer_keys):
        m, rc = self.model, self.ref_counter
        g = m.net_rows(counter.codes_of_keys(kmer_keys))
        return kernels.ref_prior_rows(rc.keys, rc.counts_by_key if rc.keys.numel() else None, kmer_keys, g, m.tau, m.net_weight,
                                      eps=epsilon, width=rc.width)


def _ref_setup(ref_model, ref_counter, counter, others):
    """The checks of ``ref_model=`` / ``ref_counter=`` (every one a ``ValueError``, before any launch) -> the ``RefModel``, or None
    where neither is given.  ``others``: the model arguments they cannot be combined with, by name."""
    if ref_model is None and ref_counter is None:
        return None
    if ref_model is None or ref_counter is None:
        raise ValueError("ref_model= and ref_counter= go together: the model and the reference column its rows are a function of")
    given = [name for name, v in others.items() if v is not None]
    if given:
        raise ValueError(f"ref_model= is the model: it cannot be combined with {', '.join(given)}")
    if not isinstance(counter, DeviceCounter) or not isinstance(ref_counter, DeviceCounter):
        raise ValueError("a reference model runs on the device only: counter= and ref_counter= must be DeviceCounters")
    if ref_counter.no_end:
        raise ValueError("ref_counter: a no_end counter; the look-up reads its keys and count rows directly")
    if counter.device != ref_counter.device:
        raise ValueError(f"counter is on {counter.device}, ref_counter on {ref_counter.device}")
    if not isinstance(ref_model, RefModel):
        ref_model = load_bear_ref(os.fspath(ref_model))[0]
    for name, c in (("counter", counter), ("ref_counter", ref_counter)):
        if (c.lag, c.alphabet_name) != (ref_model.lag, ref_model.alphabet):
            raise ValueError(f"{name}: a lag-{c.lag} table of {c.alphabet_name!r}, the model has lag {ref_model.lag} of {ref_model.alphabet!r}")
    return ref_model


class _Table:
    """The reference's DataFrame indexed by k+1-mer (get_var_probs.py:185-194) as a dense array
    ``values[kmer, letter] -> [num_models, mc_samples]`` plus the k-mer index."""

    def __init__(self, kmers, letters, values):
        self.index = {k: i for i, k in enumerate(kmers)}
        self.letter = {b: j for j, b in enumerate(letters)}
        self.values = values          # numpy [K, A+1, M, mc]
        self.lag = len(kmers[0]) if len(kmers) else 0

    def rows(self, kp1mers):
        k = np.fromiter((self.index[s[:self.lag]] for s in kp1mers), dtype=np.int64, count=len(kp1mers))
        b = np.fromiter((self.letter[s[self.lag:]] for s in kp1mers), dtype=np.int64, count=len(kp1mers))
        return self.values[k, b]      # [n, M, mc]


def df_to_func(table, num_models, mc_samples, summed=True):
    """get_var_probs.py:84-89."""
    if summed:
        return lambda kp1mers_ex: np.sum(table.rows(kp1mers_ex).reshape([-1, num_models, mc_samples]), axis=0)
    return lambda kp1mers_ex: table.rows(kp1mers_ex).reshape([-1, num_models, mc_samples])


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("bear_amd samples on an MI355X only (libbear_hip.so has no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def get_pdf(kmers, counts, h, ar_func, mc_samples, vans, train_col, alphabet_name, get_map,
            get_marg=False, summed=True, output="func", seed=None, row_base=0):
    """get_var_probs.get_pdf (get_var_probs.py:91-194).  ``kmers``: strings; ``counts``: [K, num_ds, A+1];
    ``h``: sequence of h values (used when ``ar_func`` is given); ``vans``: BMM pseudo-counts.  Returns, by
    ``output``: 'func' a function of k+1-mers -> [num_models, mc_samples] (summed) or [n, num_models, mc_samples];
    'df' a pandas DataFrame indexed by k+1-mer; 'numpy' an array [k-mer, letter, model, mc_sample]; 'device' that array as the
    CUDA tensor the sampler wrote (never copied to the host).
    With ``get_marg`` a function ``(kmers, counts) -> [num_models]`` (exact DM marginal, :155-173)."""
    assert not (get_marg and get_map), "pick marg or map"
    assert not (get_marg and output != "func"), "not implemented"
    alphabet = core.alphabets_en[alphabet_name]
    A1 = len(alphabet)
    if A1 not in kernels.WIDE_WIDTHS:
        raise NotImplementedError("the HIP kernels are built for 4-letter alphabets (+ stop): dna / rna, "
                                  "and for the protein alphabet (20 letters + stop)")
    if get_map or get_marg:
        mc_samples = 1
    device = _device()
    kmers = [k.decode() if isinstance(k, bytes) else str(k) for k in np.asarray(kmers).reshape(-1).tolist()]
    K = len(kmers)
    counts = torch.as_tensor(np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts))
    col = counts.reshape(K, -1, A1)[:, train_col, :]
    if col.dtype.is_floating_point and not torch.equal(col, col.round()):
        raise ValueError("transition counts must be integers")
    col_dev = (col.to(torch.int64) & 0xFFFFFFFF).to(torch.int32).contiguous().to(device) if K else None
    vans = np.atleast_1d(np.asarray(vans, dtype=np.float64)).reshape(-1)
    num_models = len(vans)
    prior, hs = None, np.zeros(0)
    if ar_func is not None:
        hs = np.atleast_1d(np.asarray(h, dtype=np.float64)).reshape(-1)
        num_models += len(hs)
        codes = torch.from_numpy(core.encode_kmers(kmers, alphabet_name)).to(device)
        with torch.no_grad():
            prior = ar_func(codes).to(torch.float64).expand(K, A1).contiguous()
    with_ar = ar_func is not None and get_map
    num_models += int(with_ar)

    if get_marg:
        table_index = {k: i for i, k in enumerate(kmers)}

        def prob_func(q_kmers, q_counts):
            idx = torch.as_tensor([table_index[str(k)] for k in q_kmers], dtype=torch.long, device=device)
            q = torch.as_tensor(np.asarray(q_counts), dtype=torch.int64).reshape(len(idx), A1).to(torch.int32).to(device)
            evaluate = kernels.evaluate if A1 == 5 else kernels.evaluate_wide
            out = evaluate(q.contiguous(), prior[idx].contiguous() if prior is not None else None,
                           hs if hs.size else None, vans if vans.size else None, col_dev[idx].contiguous(),
                           eps=0.0, with_ar=False).cpu().numpy()
            return np.concatenate([out[:hs.size], out[hs.size + 1:hs.size + 1 + vans.size]])
        return prob_func

    if K:
        sample = kernels.logdir_sample if A1 == 5 else kernels.logdir_sample_wide
        log_probs = sample(col_dev, prior, hs, vans, mc_samples, get_map=get_map, with_ar=with_ar,
                           seed=_next_seed() if seed is None else seed, row_base=row_base)
    else:
        log_probs = torch.zeros((0, A1, num_models, mc_samples), dtype=torch.float64, device=device)
    if output == "device":      # the sampler's table where the sampler left it (kernels.score_sum reads it there)
        return log_probs
    log_probs = log_probs.cpu().numpy()
    if output == "numpy":
        return log_probs
    table = _Table(kmers, list(alphabet), log_probs)
    if output == "df":
        import pandas as pd
        df = pd.DataFrame(log_probs.reshape(K * A1, num_models * mc_samples), index=cross_str_arrays(kmers, alphabet))
        df.columns = np.arange(len(df.columns))
        return df
    return df_to_func(table, num_models, mc_samples, summed=summed)


def make_kmc_genome_counter(path, lag, reverse=True, no_end=False):
    """get_var_probs.py:213-290 looks counts up in KMC databases through ``py_kmc_api`` (an external binary
    module, imported lazily by the reference too).  This build has no KMC: use ``make_sequence_counter`` (the same
    counts from the sequence files, counted on the device) and pass it as ``counter=``."""
    try:
        import py_kmc_api  # noqa: F401
    except ImportError as e:
        raise ImportError("make_kmc_genome_counter needs the external py_kmc_api module (KMC); build the counter "
                          "with make_sequence_counter(...) and pass it as counter=, or use the count-table path (data=...)") from e
    raise NotImplementedError("KMC database look-ups are outside this build; use make_sequence_counter")


def make_sequence_counter(seqs, lag, reverse=True, no_end=False, device=None, alphabet_name="dna"):
    """The counter of ``make_kmc_genome_counter`` (get_var_probs.py:213-290: k-mer strings -> transition counts
    ``[..., alphabet_size + 1]``) without KMC: the lag-``lag`` transition table of the sequences, counted on the device
    (``bear_amd.summarize``), as a look-up.  ``seqs``: sequences (list of str) or a summarize-style csv of
    ``FILE, GROUP, TYPE`` rows (all groups are pooled, as one KMC database is).  ``reverse`` adds the counts of the reverse
    complements (:246-248, 271-278); ``no_end`` drops the stop counts and serves only full-length contexts (:240-252).
    ``alphabet_name='prot'``: residues, rows of 21 counts, lags up to 12; there is no reverse complement, so ``reverse=False``
    has to be passed."""
    from . import summarize
    if alphabet_name == "prot" and reverse:
        raise ValueError("make_sequence_counter: the protein alphabet has no reverse complement, pass reverse=False")
    if isinstance(seqs, str):
        seqs, _ = summarize._load_sequences(seqs)
    seqs = [str(s) for s in seqs]
    text, grp = summarize.encode_sequences(seqs, [0] * len(seqs), reverse=reverse, alphabet=alphabet_name)
    kmers, counts = summarize.count_transitions(text, grp, lag, 1, device=device, alphabet=alphabet_name)
    table = {bytes(k).decode(): counts[0, i].astype(np.float64) for i, k in enumerate(kmers)}
    A1 = counts.shape[-1]

    def counter(kmers):
        kmers = np.asarray(kmers)
        out = np.zeros((kmers.size, A1))
        for i, k in enumerate(kmers.reshape(-1).tolist()):
            k = k.decode() if isinstance(k, bytes) else str(k)
            if no_end and "[" in k:
                continue
            row = table.get(k)
            if row is not None:
                out[i] = row
        if no_end:
            out[:, -1] = 0
        return out.reshape(kmers.shape + (A1,))
    return counter


# ------------------------------------------------------------------------------------------- scoring on the device
_NO_SYMBOL = 0xFE      # the code of a character outside the alphabet (beyond every symbol code: the kernel makes no key of it)


def _symbol_lut(alphabet_name):
    """byte -> symbol code of the scoring text (include/bear_hip.h): letters 0 .. W - 2, ']' W - 1, '[' W, anything else _NO_SYMBOL."""
    alphabet = core.alphabets_en[alphabet_name]
    lut = np.full(256, _NO_SYMBOL, dtype=np.uint8)
    for c, ch in enumerate(alphabet):
        lut[ord(ch)] = c
    lut[ord("[")] = len(alphabet)
    return lut


class _KeyLookup:
    """What ``DeviceCounter`` and ``classify.GroupCounter`` share: the k-mers of a table in HBM as a look-up -- ``kmers`` uint8
    [N, lag] (ASCII) and their keys sorted once (``keys`` int64 [N'] ascending, ``perm`` their rows)."""

    _counts_shape = "[N, W]"          # the counts a subclass holds per k-mer: the first axis is the k-mers', the last has W entries

    def _build_lookup(self, kmers, counts, alphabet_name, no_end):
        if not (isinstance(kmers, torch.Tensor) and kmers.is_cuda and kmers.dtype == torch.uint8 and kmers.dim() == 2):
            raise ValueError("kmers must be a CUDA uint8 tensor [N, lag] of ASCII k-mers")
        if not (isinstance(counts, torch.Tensor) and counts.device == kmers.device and counts.dtype == torch.int32
                and counts.dim() == len(self._counts_shape.split(",")) and counts.shape[0] == kmers.shape[0]):
            raise ValueError(f"counts must be a CUDA int32 tensor {self._counts_shape} on the k-mers' device")
        self.alphabet_name, self.no_end = alphabet_name, bool(no_end)
        self.rank = kernels.score_ranks(alphabet_name)
        self.width, self.lag = len(self.rank) - 1, int(kmers.shape[1])
        if counts.shape[-1] != self.width:
            raise ValueError(f"counts: rows of {counts.shape[-1]}, the alphabet {alphabet_name!r} has rows of {self.width}")
        if not 1 <= self.lag <= kernels.SCORE_MAX_LAG[self.width]:
            raise ValueError(f"lag {self.lag}: a look-up key holds contexts of 1..{kernels.SCORE_MAX_LAG[self.width]} letters of {alphabet_name!r}")
        self.kmers, self.counts = kmers.contiguous(), counts.contiguous()
        self._lut = _symbol_lut(alphabet_name)
        keys = self._keys_of_codes(torch.from_numpy(self._lut).to(kmers.device)[self.kmers.long()])
        held = torch.nonzero(keys >= 0).reshape(-1)
        self.keys, order = torch.sort(keys[held])
        self.perm = held[order]
        if self.keys.numel() > 1 and bool((self.keys[1:] == self.keys[:-1]).any()):
            raise ValueError(f"{type(self).__name__}: the table holds a k-mer twice")

    @property
    def device(self):
        return self.kmers.device

    def _keys_of_codes(self, codes):
        """Keys int64 [n] of k-mers given as symbol codes uint8 [n, lag] on the device (-1: a symbol that is no letter of a context):
        every k-mer becomes a segment of lag + 1 symbols, the k-mer and a stop, whose one transition carries the k-mer's key."""
        n = codes.shape[0]
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=codes.device)
        text = torch.cat([codes, torch.full((n, 1), self.width - 1, dtype=torch.uint8, device=codes.device)], 1).reshape(-1)
        seg = torch.arange(n + 1, dtype=torch.int64, device=codes.device) * (self.lag + 1)
        keys, _ = kernels.score_transitions(text, seg, self.lag, self.rank)
        return keys.reshape(n, self.lag + 1)[:, self.lag].contiguous()

    def _find(self, keys):
        """Per key (int64 [n] on the device) ``(idx int64, keep bool)``: its place in ``perm`` (0 where it is absent) and whether its
        counts are to be read at all -- not for an absent k-mer, nor, under ``no_end``, for a context that holds ``[``."""
        idx = kernels.kmer_find(self.keys, keys.contiguous())
        keep = idx >= 0
        if self.no_end:
            bits, start = kernels.SCORE_BITS[self.width], int(self.rank[self.width])
            shifts = torch.arange(self.lag, dtype=torch.int64, device=self.device) * bits
            keep = keep & ~(((keys[:, None] >> shifts[None, :]) & ((1 << bits) - 1)) == start).any(1)
        return idx.clamp(min=0).long(), keep

    def rows_of_keys(self, keys):
        """Count rows int32 [n, W] (``counts`` [N, G, W]: [n, G, W]) of the k-mers with the given keys (int64 [n] on the device;
        ascending is the fast order): zeros for an absent k-mer; under ``no_end`` also for a context that holds ``[``, and in the
        stop column."""
        idx, keep = self._find(keys)
        rows = self.counts[self.perm[idx]] if self.keys.numel() else \
            torch.zeros((keys.numel(),) + tuple(self.counts.shape[1:]), dtype=torch.int32, device=self.device)
        rows = rows * keep.reshape((-1,) + (1,) * (rows.dim() - 1)).to(torch.int32)
        if self.no_end:
            rows[..., -1] = 0
        return rows.contiguous()

    def codes_of_keys(self, keys):
        """``core.encode_kmers`` codes int8 [n, lag] (letters 0 .. A - 1, ``[`` = A) of the k-mers with the given valid keys."""
        bits = kernels.SCORE_BITS[self.width]
        code_of_rank = np.zeros(1 << bits, dtype=np.int8)
        code_of_rank[self.rank[:self.width - 1]] = np.arange(self.width - 1)
        code_of_rank[self.rank[self.width]] = self.width - 1
        shifts = torch.arange(self.lag - 1, -1, -1, dtype=torch.int64, device=self.device) * bits
        ranks = (keys[:, None] >> shifts[None, :]) & ((1 << bits) - 1)
        return torch.from_numpy(code_of_rank).to(self.device)[ranks].contiguous()


class DeviceCounter(_KeyLookup):
    """The pooled lag-``lag`` transition table of one dataset column in HBM, as a look-up: ASCII k-mers ``kmers`` uint8 [N, lag],
    ``counts`` [N, W] (uint32 in int32 storage), and the k-mers' keys sorted once (``keys`` int64 [N'] ascending, ``perm`` their
    rows; a k-mer with a character outside the alphabet has no key and is never found).  A key packs the ranks of a k-mer's
    characters in byte order, first letter most significant (``kernels.score_ranks``), so keys sort as Python sorts the strings.

    Called with k-mer strings it returns what ``make_sequence_counter``'s closure returns, ``no_end`` included, so it is a valid
    ``counter=`` anywhere.  Handed to ``get_bear_probs`` / ``get_bear_probs_seqs`` (without ``get_marg``) the whole call runs on the
    device: keys of the queries' transitions, their distinct k-mers, count rows by ``kernels.kmer_find``, the sampled or MAP table
    and the per-variant / per-sequence sums (``kernels.score_sum``); only the scores come back.  ``train_col`` of those calls is
    not used then: the counter is one column.  ``get_marg=True`` runs on the device too when ``marg_on_device=True`` is passed
    with it (``kernels.score_marg``); by default that one mode calls the counter per k-mer on the host.  Handed to ``assemble.assemble_no_ends`` the flanks grow on the device
    (``kernels.generate_steps`` over ``keys`` and ``counts_by_key``); handed to ``assemble.generate_sequences`` (counted with ends:
    ``no_end=False``) whole sequences are sampled from the start context to the stop (``kernels.generate_whole``)."""

    def __init__(self, kmers, counts, alphabet_name, no_end=False):
        self._build_lookup(kmers, counts, alphabet_name, no_end)

    @property
    def counts_by_key(self):
        """The count rows in key order, int32 [N', W] with row j the counts of ``keys[j]`` (``counts[perm]``): what
        ``kernels.generate_steps`` looks rows up in.  Built on first use and kept."""
        if getattr(self, "_counts_by_key", None) is None:
            self._counts_by_key = self.counts[self.perm].contiguous()
        return self._counts_by_key

    def __call__(self, kmers):
        kmers = np.asarray(kmers)
        flat = [k.decode() if isinstance(k, bytes) else str(k) for k in kmers.reshape(-1).tolist()]
        out = np.zeros((len(flat), self.width))
        sized = [i for i, k in enumerate(flat) if len(k) == self.lag]
        if sized:
            raw = np.frombuffer("".join(flat[i] for i in sized).encode("ascii", "replace"), dtype=np.uint8)
            keys = self._keys_of_codes(torch.from_numpy(self._lut[raw].reshape(len(sized), self.lag)).to(self.device))
            rows = self.rows_of_keys(keys)
            out[sized] = (rows.to(torch.int64) & 0xFFFFFFFF).to(torch.float64).cpu().numpy()
        return out.reshape(kmers.shape + (self.width,))

    @classmethod
    def from_sequences(cls, seqs, lag, reverse=True, no_end=False, device=None, alphabet_name="dna"):
        """``make_sequence_counter``'s arguments; the table is counted with ``summarize.count_transitions(..., on_device=True)`` and
        stays where it was counted."""
        from . import summarize
        if alphabet_name == "prot" and reverse:
            raise ValueError("DeviceCounter.from_sequences: the protein alphabet has no reverse complement, pass reverse=False")
        if isinstance(seqs, str):
            seqs, _ = summarize._load_sequences(seqs)
        seqs = [str(s) for s in seqs]
        text, grp = summarize.encode_sequences(seqs, [0] * len(seqs), reverse=reverse, alphabet=alphabet_name)
        kmers, counts = summarize.count_transitions(text, grp, lag, 1, device=device, on_device=True, alphabet=alphabet_name)
        return cls(kmers, counts[0], alphabet_name, no_end=no_end)

    @classmethod
    def from_dataset(cls, data, train_col, no_end=False, device=None):
        """Column ``train_col`` of a ``CountDataset`` (uploaded) or a ``DeviceCountDataset`` (in place), e.g. ``load_bear(path)[4]``."""
        if getattr(data, "shard", None) is not None:
            raise ValueError("DeviceCounter.from_dataset: a row-sharded table holds only one rank's k-mers")
        if isinstance(data, dataloader.DeviceCountDataset):
            return cls(data.kmers_dev, data.counts_dev[int(train_col)], data.alphabet, no_end=no_end)
        device = _device() if device is None else torch.device(device)
        kmers = torch.from_numpy(np.ascontiguousarray(data.kmers, dtype=np.uint8)).to(device)
        counts = torch.from_numpy(np.ascontiguousarray(data.counts[int(train_col)]).view(np.int32)).to(device)
        return cls(kmers, counts, data.alphabet, no_end=no_end)


def _segment_text(segments, lag, alphabet_name):
    """Strings -> ``(codes uint8 [n_sym], offsets int64 [n_seg + 1], positions without a transition)`` of the scoring text.  What the
    kernels would make no key of is refused here, before any launch: a character outside the alphabet, a ``]`` inside a context,
    a ``[`` as a next symbol."""
    lut = _symbol_lut(alphabet_name)
    W = len(core.alphabets_en[alphabet_name])
    lens = np.fromiter((len(s) for s in segments), dtype=np.int64, count=len(segments))
    joined = "".join(segments)
    codes = lut[np.frombuffer(joined.encode("ascii", "replace"), dtype=np.uint8)]
    bad = np.flatnonzero(codes == _NO_SYMBOL)
    if bad.size:
        raise ValueError(f"character {joined[bad[0]]!r} is not a letter of the alphabet {alphabet_name!r}, '[' or ']'")
    seg = np.zeros(len(segments) + 1, dtype=np.int64)
    np.cumsum(lens, out=seg[1:])
    pos = np.arange(codes.size, dtype=np.int64) - np.repeat(seg[:-1], lens)
    seg_len = np.repeat(lens, lens)
    in_context = (seg_len > lag) & (pos < seg_len - 1)
    if np.any(in_context & (codes == W - 1)):
        raise ValueError("character ']' inside a context: the stop symbol can only end a sequence")
    if np.any((pos >= lag) & (codes == W)):
        raise ValueError("character '[' behind a context: the start symbol can only pad the front of a sequence")
    return codes, seg, int(np.minimum(lens, lag).sum())


def _free_memory(device):
    """Bytes a call can still take on ``device``: what the driver reports plus what torch's allocator caches."""
    return torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def _segment_rows(counter, segments, lag, alphabet_name, h, ar_func, vans):
    """What ``_score_segments`` and ``_marg_segments`` do alike, up to their memory figure: the refusals, the scoring text, its keys,
    the distinct k-mers -- numbered as ``np.array(sorted(set(all_kmers)))`` numbers them (ascending keys) -- and the row of every
    position -> ``(hs, vans, text)``, ``text`` = ``(seg, rows, letters, kmer_keys, positions)``, tensors on the device, or None
    where there is no transition anywhere.  (``ar_func``: anything but None says "with BEAR models"; it is not called here.)"""
    if counter.lag != lag or counter.alphabet_name != alphabet_name:
        raise ValueError(f"counter: a lag-{counter.lag} table of {counter.alphabet_name!r}, asked for lag {lag} of {alphabet_name!r}")
    device = counter.device
    vans = np.atleast_1d(np.asarray(vans, dtype=np.float64)).reshape(-1)
    hs = np.atleast_1d(np.asarray(h, dtype=np.float64)).reshape(-1) if ar_func is not None else np.zeros(0)
    codes, seg, n_none = _segment_text(segments, lag, alphabet_name)
    if codes.size == n_none:
        return hs, vans, None
    with torch.cuda.device(device):
        seg = torch.from_numpy(seg).to(device)
        keys, letters = kernels.score_transitions(torch.from_numpy(codes).to(device), seg, lag, counter.rank)
        uniq, inverse = torch.unique(keys, return_inverse=True)     # ascending; -1 (no transition) in front where there is one
        first = int(n_none > 0)
        return hs, vans, (seg, (inverse - first).to(torch.int32), letters, uniq[first:].contiguous(), codes.size)


def _prior_rows(counter, ar_func, kmer_keys, need, what, advice):
    """The AR function's rows [K, W] of the distinct k-mers (None without one), formed only once the caller's ``need`` bytes are
    known to fit the free device memory: otherwise ``MemoryError``, before the AR function is called."""
    free = _free_memory(counter.device)
    if need > free:
        raise MemoryError(f"{what} {need} bytes, the device has {free} free: {advice}")
    if ar_func is None:
        return None
    if isinstance(ar_func, _RefRows):
        return ar_func.rows(counter, kmer_keys)
    with torch.no_grad():
        return ar_func(counter.codes_of_keys(kmer_keys)).to(torch.float64).expand(kmer_keys.numel(), counter.width).contiguous()


def _score_segments(counter, segments, lag, alphabet_name, h, ar_func, mc_samples, vans, get_map, seed):
    """The device path of get_bear_probs / get_bear_probs_seqs: ``scores[i] = sum of log p(next | k-mer)`` over the transitions of
    string ``i`` -> CUDA float64 [n_seg, num_models, mc_samples].  The number of a distinct k-mer (``_segment_rows``) keys the
    sampler's draws: with equal ``seed`` the table is the one the host ``counter=`` path samples.

    The table ``[K, W, num_models, mc_samples]`` is held whole: if it would not fit the free device memory a ``MemoryError`` says
    so (score fewer strings or samples per call) -- rows are not processed in pieces, so a result never depends on what else
    the device holds."""
    hs, vans, text = _segment_rows(counter, segments, lag, alphabet_name, h, ar_func, vans)
    with_ar = ar_func is not None and get_map
    num_models = len(vans) + len(hs) + int(with_ar)
    if get_map:
        mc_samples = 1
    if text is None:                # no transition anywhere
        return torch.zeros((len(segments), num_models, mc_samples), dtype=torch.float64, device=counter.device)
    seg, rows, letters, kmer_keys, _ = text
    K, W = kmer_keys.numel(), counter.width
    with torch.cuda.device(counter.device):
        prior = _prior_rows(counter, ar_func, kmer_keys, K * W * num_models * mc_samples * 8,
                            f"the sampled table of {K} k-mers x {W} letters x {num_models} models x {mc_samples} samples takes",
                            "score fewer variants / sequences or samples per call")
        sample = kernels.logdir_sample if W == 5 else kernels.logdir_sample_wide
        lp = sample(counter.rows_of_keys(kmer_keys), prior, hs, vans, mc_samples, get_map=get_map, with_ar=with_ar, seed=seed,
                    row_base=0)
        return kernels.score_sum(lp, rows, letters, seg)


def _marg_segments(counter, segments, lag, alphabet_name, h, ar_func, vans):
    """The device path of ``get_bear_probs_seqs(..., get_marg=True, marg_on_device=True)``: the exact Dirichlet-multinomial marginal
    of string ``i`` under every model -> CUDA float64 [n_seg, num_models], BEAR models first.  ``_segment_rows`` and ``_prior_rows``
    -- the refusals, keys, distinct k-mers and prior rows of ``_score_segments`` -- then the count rows and ``kernels.score_marg``
    instead of a table.

    Per distinct k-mer the call holds a count row, a prior row and the rows' gather temporaries, per position one term per model:
    if that would not fit the free device memory a ``MemoryError`` says so, as ``_score_segments`` does."""
    hs, vans, text = _segment_rows(counter, segments, lag, alphabet_name, h, ar_func, vans)
    num_models = len(vans) + len(hs)
    if text is None:                # no transition anywhere
        return torch.zeros((len(segments), num_models), dtype=torch.float64, device=counter.device)
    seg, rows, letters, kmer_keys, positions = text
    K, W = kmer_keys.numel(), counter.width
    with torch.cuda.device(counter.device):
        prior = _prior_rows(counter, ar_func, kmer_keys, K * W * 3 * 8 + positions * (num_models * 8 + 3 * 8),
                            f"the rows of {K} k-mers x {W} letters and the terms of {positions} positions x {num_models} models take",
                            "score fewer sequences per call")
        return kernels.score_marg(rows, letters, seg, counter.rows_of_keys(kmer_keys), prior, hs, vans)


def _check_moments(counter, **others):
    """The refusals of ``moments=True`` (every one a ``ValueError``, before a device is touched): it is the device path's, and
    ``others`` -- by name -- are the results it cannot be combined with."""
    if not isinstance(counter, DeviceCounter):
        raise ValueError("moments=True runs on the device only: counter= must be a DeviceCounter")
    given = [name for name, v in others.items() if v]
    if given:
        raise ValueError(f"moments=True is the mean and variance of the sampled scores: it cannot be combined with {', '.join(given)}")


def _signed_pairs(seg):
    """Windows in pairs (mutant, wild type) -> one signed segment per pair: ``seg`` int64 [2 n + 1], the windows' offsets ->
    ``(seg[0::2], weights int8 [seg[-1]])``, +1 on the positions of every mutant window and -1 on the wild type's.  The transitions
    are formed under the windows' own offsets (``_segment_rows``): none crosses from one window of a pair into the other."""
    seg = np.asarray(seg, dtype=np.int64)
    assert seg.size % 2 == 1
    sign = np.tile(np.array([1, -1], dtype=np.int8), seg.size // 2)
    return seg[0::2].copy(), np.repeat(sign, np.diff(seg))


def _moment_segments(counter, segments, lag, alphabet_name, h, ar_func, vans, pair=False):
    """The device path of ``moments=True``: the exact mean and variance, over the posterior the sampled path draws from, of the score
    of string ``i`` under every model -> CUDA float64 [n_seg, num_models, 2] (variance as summed), BEAR models first.
    ``_segment_rows`` and ``_prior_rows`` as ``_marg_segments`` calls them, then ``kernels.score_moments``.  ``pair``: the strings
    are windows in pairs (mutant, wild type) and a pair is ONE signed segment (``_signed_pairs``) -> [n_seg / 2, num_models, 2].

    Per distinct k-mer the call holds what ``_marg_segments`` holds, per position two terms per model, the sort's key and order,
    the weight's prefix sum and the rows: if that would not fit the free device memory a ``MemoryError`` says so.  There is no
    sampled table."""
    hs, vans, text = _segment_rows(counter, segments, lag, alphabet_name, h, ar_func, vans)
    num_models = len(vans) + len(hs)
    n_out = len(segments) // 2 if pair else len(segments)
    if text is None:                # no transition anywhere
        return torch.zeros((n_out, num_models, 2), dtype=torch.float64, device=counter.device)
    seg, rows, letters, kmer_keys, positions = text
    K, W = kmer_keys.numel(), counter.width
    with torch.cuda.device(counter.device):
        prior = _prior_rows(counter, ar_func, kmer_keys, K * W * 3 * 8 + positions * (2 * num_models + 4) * 8,
                            f"the rows of {K} k-mers x {W} letters and the terms of {positions} positions x 2 x {num_models} models take",
                            "score fewer variants / sequences per call")
        weights = None
        if pair:
            coarse, weights = _signed_pairs(seg.cpu().numpy())
            seg, weights = torch.from_numpy(coarse).to(counter.device), torch.from_numpy(weights).to(counter.device)
        return kernels.score_moments(rows, letters, seg, counter.rows_of_keys(kmer_keys), prior, hs, vans, weights=weights)


def _moments_result(moments):
    """What ``moments=True`` returns: NumPy float64 [n, num_models, 2], the variance -- a sum that rounding can leave a few ulps
    below 0 -- not below 0 (its user takes a square root)."""
    out = moments.cpu().numpy()
    np.maximum(out[..., 1], 0.0, out=out[..., 1])
    return out


def _variant_windows(vars_, wt_seq, lag):
    """Per variant its two windows, the mutant's then the wild type's (get_var_probs.py:294-306): ``wt_seq`` padded, ``vars_`` parsed."""
    windows = []
    for wt_aa, mt_aa, pos in vars_:
        pos = pos + lag
        assert wt_aa == wt_seq[pos:pos + len(wt_aa)]
        windows.append(wt_seq[pos - lag:pos] + mt_aa + wt_seq[pos + len(wt_aa):pos + lag + len(wt_aa)])
        windows.append(wt_seq[pos - lag:pos + lag + len(wt_aa)])
    return windows


# ------------------------------------------------------------------------------------------- variants
def _add_kmer_probs_vars(vars_, scores, wt_seq, pdf, lag, seen_kmers):
    """get_var_probs.py:294-306."""
    seen = set(np.asarray(seen_kmers).astype(str).tolist())
    for i, (wt_aa, mt_aa, pos) in enumerate(vars_):
        pos = pos + lag
        assert wt_aa == wt_seq[pos:pos + len(wt_aa)]
        wt_win = wt_seq[pos - lag:pos + lag + len(wt_aa)]
        wt_kmers = [wt_win[j:j + lag + 1] for j in range(len(wt_win) - lag) if wt_win[j:j + lag] in seen]
        mt_win = wt_seq[pos - lag:pos] + mt_aa + wt_seq[pos + len(wt_aa):pos + lag + len(wt_aa)]
        mt_kmers = [mt_win[j:j + lag + 1] for j in range(len(mt_win) - lag) if mt_win[j:j + lag] in seen]
        scores[i, :, :] += pdf(mt_kmers) - pdf(wt_kmers)
    return scores


def _get_all_kmers_vars(vars_, wt_seq, lag):
    """get_var_probs.py:309-337."""
    all_kmers = []
    for (wt_aa, mt_aa, pos) in vars_:
        pos = pos + lag
        assert wt_aa == wt_seq[pos:pos + len(wt_aa)]
        wt_win = wt_seq[pos - lag:pos + lag + len(wt_aa)]
        mt_win = wt_seq[pos - lag:pos] + mt_aa + wt_seq[pos + len(wt_aa):pos + lag + len(wt_aa)]
        all_kmers += [wt_win[j:j + lag] for j in range(len(wt_win) - lag)]
        all_kmers += [mt_win[j:j + lag] for j in range(len(mt_win) - lag)]
    return np.array(sorted(set(all_kmers))).astype(str)


def parse_var(var):
    """'AAG23CC' -> ('AAG', 'CC', 23) (get_var_probs.py:339-344)."""
    digits = [i for i, ch in enumerate(var) if ch.isnumeric()]      # (plain Python: a tenth of the time of the NumPy form, which was most of a device-path call)
    if not digits:
        raise ValueError(f"variant {var!r} holds no position")
    pos_num, len_num = digits[0], len(digits)
    return (var[:pos_num], var[pos_num + len_num:], int(var[pos_num:pos_num + len_num]))


def _scan(data, all_kmers, add, make_pdf, alphabet_size, train_col):
    """The batch loop shared by get_bear_probs / get_bear_probs_seqs (get_var_probs.py:421-447, 598-626):
    every batch contributes the k-mers it holds; k-mers never seen contribute through the prior alone."""
    seen_all = np.zeros(len(all_kmers))
    row0 = 0
    for kmers, counts in iter(data):
        kmers = np.asarray(kmers).astype(str)
        in_kmers = np.isin(kmers, all_kmers)
        if np.sum(in_kmers) > 0:
            seen_kmers = kmers[in_kmers]
            seen_counts = np.asarray(counts)[in_kmers]
            seen_all += np.isin(all_kmers, seen_kmers)
            add(make_pdf(seen_kmers, seen_counts, row0), seen_kmers)
        row0 += len(kmers)
    unseen = seen_all == 0
    if np.sum(unseen) > 0:
        add(make_pdf(all_kmers[unseen], np.zeros([int(np.sum(unseen)), train_col + 1, alphabet_size + 1]), row0),
            all_kmers[unseen].astype(str))


def _setup(bear_path, lag, alphabet_name, h, data, vans, kmc_path, counter=None, ref_model=None, ref_counter=None):
    ref_model = _ref_setup(ref_model, ref_counter, counter, dict(bear_path=bear_path))
    if ref_model is not None:       # a bear_ref model: its rows come from kernels.ref_prior_rows (_prior_rows)
        h = np.array([ref_model.h]) if h is None else np.atleast_1d(h)
        return ref_model.lag, ref_model.alphabet, h, _RefRows(ref_model, ref_counter), data, len(h)
    if bear_path is not None:
        lag, alphabet_name, h_bear, ar_func, data = load_bear(bear_path)
        if h is None:
            h = np.array([h_bear])
        len_h = len(h)
    else:
        assert ((lag is not None and alphabet_name is not None)
                and ((data is not None or kmc_path is not None or counter is not None) and len(vans) > 0))
        len_h, ar_func = 0, None
    if kmc_path is not None and counter is None:
        make_kmc_genome_counter(kmc_path, lag)
    return lag, alphabet_name, h, ar_func, data, len_h


def get_bear_probs(bear_path, wt_seq, vars_, train_col, mc_samples=41, vans=[0.1, 1, 10], get_map=False,
                   lag=None, alphabet_name=None, h=None, data=None, kmc_path=None, kmc_reverse=False,
                   kmc_no_end=False, seed=None, counter=None, ref_model=None, ref_counter=None, moments=False):
    """get_var_probs.get_bear_probs (get_var_probs.py:346-452): posterior predictive log-probability ratios of
    variants -> [num variants, num models, mc_samples] ([num variants, num models] with ``get_map``).

    ``ref_model=`` (a ``RefModel`` or a folder of ``train_bear_ref.py``) with ``ref_counter=`` (the ``DeviceCounter`` of the reference
    column) scores under a model trained by ``bear_ref``, on the device: ``counter`` must be a ``DeviceCounter`` too, ``bear_path`` None.

    ``moments=True`` (with a ``DeviceCounter``, without ``get_map``; anything else is a ``ValueError``, raised before a device is
    touched): instead of ``mc_samples`` draws, the exact mean and variance of what that axis samples -> float64 [num variants, num
    models, 2], ``[..., 0]`` the mean and ``[..., 1]`` the variance (not below 0), the models in the sampled path's order.  Closed
    form (digamma and trigamma of the posterior's concentrations, ``kernels.score_moments``): no Monte-Carlo noise, the same
    result whatever ``seed``, ``mc_samples`` and the other variants of the call are, and no sampled table in memory."""
    if moments:
        _check_moments(counter, get_map=get_map)
    lag, alphabet_name, h, ar_func, data, len_h = _setup(bear_path, lag, alphabet_name, h, data, vans, kmc_path, counter,
                                                         ref_model, ref_counter)
    alphabet_size = len(core.alphabets_en[alphabet_name]) - 1
    wt_seq = lag * "[" + wt_seq + "]"
    vars_ = [parse_var(v) for v in vars_]
    if get_map:
        mc_samples = 1
    num_models = (ar_func is not None) * (len_h + get_map) + len(vans)
    scores = np.zeros([len(vars_), num_models, mc_samples])
    seed = _next_seed() if seed is None else seed
    if moments:                                 # a variant is ONE signed segment: its mutant window counts +1, its wild type's -1
        windows = _variant_windows(vars_, wt_seq, lag)
        if not windows:
            return np.zeros([0, num_models, 2])
        return _moments_result(_moment_segments(counter, windows, lag, alphabet_name, h, ar_func, vans, pair=True))
    if isinstance(counter, DeviceCounter):      # the whole call on the device: a variant is two segments, mutant and wild-type window
        windows = _variant_windows(vars_, wt_seq, lag)
        if windows:
            sums = _score_segments(counter, windows, lag, alphabet_name, h, ar_func, mc_samples, vans, get_map, seed)
            scores = (sums[0::2] - sums[1::2]).cpu().numpy()
        return scores[..., 0] if get_map else scores
    all_kmers = _get_all_kmers_vars(vars_, wt_seq, lag)

    def make_pdf(kmers, counts, row0):
        return get_pdf(kmers, counts, h, ar_func, mc_samples, vans, train_col, alphabet_name, get_map, seed=seed, row_base=row0)

    def add(pdf, seen):
        _add_kmer_probs_vars(vars_, scores, wt_seq, pdf, lag, seen)
    if counter is not None:     # get_var_probs.py:411-420: counts looked up per k-mer instead of scanning the table
        add(make_pdf(all_kmers, counter(all_kmers)[:, None, :], 0), all_kmers)
    else:
        _scan(data, all_kmers, add, make_pdf, alphabet_size, train_col)
    return scores[..., 0] if get_map else scores


# ------------------------------------------------------------------------------------------- whole sequences
def _add_kmer_probs_seqs(seqs, scores, pdf, lag, seen_kmers, get_marg, alphabet):
    """get_var_probs.py:455-482."""
    seen = set(np.asarray(seen_kmers).astype(str).tolist())
    if get_marg:
        for i, seq in enumerate(seqs):
            kp1 = [(seq[l:l + lag], alphabet == seq[l + lag]) for l in range(len(seq) - lag) if seq[l:l + lag] in seen]
            if kp1:
                kmers_red = np.array([k for k, _ in kp1])
                counts_red = np.array([b for _, b in kp1]).astype(int)
                kmers, maps = np.unique(kmers_red, return_inverse=True)
                counts = np.zeros((len(kmers), len(alphabet)), dtype=int)
                np.add.at(counts, maps, counts_red)          # transitions of a repeated k-mer add up (:471-473)
                scores[i, :, 0] += pdf(kmers, counts)
    else:
        for i, seq in enumerate(seqs):
            kp1mers = [seq[l:l + lag + 1] for l in range(len(seq) - lag) if seq[l:l + lag] in seen]
            scores[i, :, :] += pdf(kp1mers)
    return scores


def _get_all_kmers_seqs(seqs, lag):
    """get_var_probs.py:484-508."""
    all_kmers = set()
    for seq in seqs:
        assert len(seq.replace("[", "").replace("]", "")) >= lag
        all_kmers.update(seq[j:j + lag] for j in range(len(seq) - lag))
    return np.array(sorted(all_kmers)).astype(str)


def get_bear_probs_seqs(bear_path, seqs, train_col, mc_samples=41, vans=[0.1, 1, 10], get_map=False, get_marg=False,
                        lag=None, alphabet_name=None, h=None, data=None, kmc_path=None, kmc_reverse=False,
                        no_ends=False, seed=None, counter=None, marg_on_device=False, ref_model=None, ref_counter=None,
                        moments=False):
    """get_var_probs.get_bear_probs_seqs (get_var_probs.py:511-631): log-probabilities of whole sequences ->
    [num sequences, num models, mc_samples] (last axis dropped with ``get_map`` / ``get_marg``).

    ``marg_on_device=True`` (with ``get_marg=True`` and a ``DeviceCounter``; anything else is a ``ValueError``, raised before a
    device is touched): the exact marginals are formed on the device from the sequences' symbols to the scores
    (``_marg_segments``, ``kernels.score_marg``) -> [num sequences, num models].  The default stays ``False``, the host loop with
    the counter called per k-mer: the device sums a sequence's terms in another order, so its scores agree with the host loop's
    to rounding (1e-11 of the terms' L1 mass is what the tests hold it to), not to the bit, and the bits of the default are
    pinned.  Making the device path the default is a later decision.

    ``ref_model=`` / ``ref_counter=``: as for ``get_bear_probs``; ``get_marg=True`` then needs ``marg_on_device=True`` (a reference
    model has no host path).

    ``moments=True``: as for ``get_bear_probs`` -> float64 [num sequences, num models, 2], the exact mean and variance of what the
    ``mc_samples`` axis samples; a ``ValueError`` together with ``get_map``, ``get_marg`` or ``marg_on_device`` or without a
    ``DeviceCounter``."""
    if moments:
        _check_moments(counter, get_map=get_map, get_marg=get_marg, marg_on_device=marg_on_device)
    if marg_on_device and not (get_marg and isinstance(counter, DeviceCounter)):
        raise ValueError("marg_on_device=True is the device path of get_marg=True with a DeviceCounter as counter=")
    if (ref_model is not None or ref_counter is not None) and get_marg and not marg_on_device:
        raise ValueError("a reference model runs on the device only: get_marg=True needs marg_on_device=True with it")
    lag, alphabet_name, h, ar_func, data, len_h = _setup(bear_path, lag, alphabet_name, h, data, vans, kmc_path, counter,
                                                         ref_model, ref_counter)
    alphabet = core.alphabets_en[alphabet_name]
    alphabet_size = len(alphabet) - 1
    if not no_ends:
        seqs = [lag * "[" + s + "]" for s in seqs]
    if get_map or get_marg:
        mc_samples = 1
    num_models = (ar_func is not None) * (len_h + get_map) + len(vans)
    scores = np.zeros([len(seqs), num_models, mc_samples])
    seed = _next_seed() if seed is None else seed
    if moments:                                                 # the exact moments on the device: a sequence is a segment
        for seq in seqs:
            assert len(seq.replace("[", "").replace("]", "")) >= lag
        if not len(seqs):
            return np.zeros([0, num_models, 2])
        return _moments_result(_moment_segments(counter, seqs, lag, alphabet_name, h, ar_func, vans))
    if marg_on_device:                                          # the exact marginal on the device: a sequence is a segment
        for seq in seqs:
            assert len(seq.replace("[", "").replace("]", "")) >= lag
        if len(seqs):
            return _marg_segments(counter, seqs, lag, alphabet_name, h, ar_func, vans).cpu().numpy()
        return scores[..., 0]
    if isinstance(counter, DeviceCounter) and not get_marg:     # the whole call on the device: a sequence is a segment
        for seq in seqs:
            assert len(seq.replace("[", "").replace("]", "")) >= lag
        if len(seqs):
            scores = _score_segments(counter, seqs, lag, alphabet_name, h, ar_func, mc_samples, vans, get_map, seed).cpu().numpy()
        return scores[..., 0] if get_map else scores
    all_kmers = _get_all_kmers_seqs(seqs, lag)

    def make_pdf(kmers, counts, row0):
        return get_pdf(kmers, counts, h, ar_func, mc_samples, vans, train_col, alphabet_name, get_map, get_marg,
                       seed=seed, row_base=row0)

    def add(pdf, seen):
        _add_kmer_probs_seqs(seqs, scores, pdf, lag, seen, get_marg, alphabet)
    if counter is not None:     # get_var_probs.py:585-597
        add(make_pdf(all_kmers, counter(all_kmers)[:, None, :], 0), all_kmers)
    else:
        _scan(data, all_kmers, add, make_pdf, alphabet_size, train_col)
    return scores[..., 0] if (get_map or get_marg) else scores
