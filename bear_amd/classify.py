"""Which group of a count table does a sequence belong to?  The exact Dirichlet-multinomial marginal of every sequence under the
posterior of EVERY group (column) of one table, in one pass over the sequences (``bear_score_groups_f64``, kernels_groups.h), and
the posterior over the groups that follows from it.

The sequences are encoded once, their distinct k-mers looked up once and the AR function evaluated once: its rows depend on the
k-mer only, so one function serves all groups; only the count row differs between them.  A sequence that is itself in the table
(judging a classifier on its training sequences) is scored under its own group with its own transitions taken out of that
group's counts first -- the leave-one-out marginal, which no look-up can give because the removal differs for every sequence.
Nothing here computes but ``log_post``, a logsumexp over the groups in plain torch on the device.

And WHERE in a sequence which group speaks: ``position_log_probs`` -- the posterior-predictive log-probability of every
transition's letter under every group (``bear_score_emit_groups_f64``) -- and ``segment`` -- a hidden-Markov chain over the groups
on those emissions (``bear_hmm_groups_f64``, kernels_segment.h): the best path, every position's posterior over the groups and the
evidence."""
import numpy as np
import torch

from . import dataloader, get_var_probs, hypothesis, kernels


class GroupCounter(get_var_probs._KeyLookup):
    """The lag-``lag`` transition table of G groups in HBM, as one look-up: ASCII k-mers ``kmers`` uint8 [N, lag], the shared
    ``keys`` / ``perm`` that ``DeviceCounter`` builds for one column, and ``counts`` int32 [N, G, W] (uint32 in int32 storage), the G
    count rows of a k-mer adjacent.  ``reverse``: the table also holds every sequence's reverse complement (``from_sequences``
    remembers it; a table from a dataset is taken to hold forward transitions only)."""
    _counts_shape = "[N, G, W]"

    def __init__(self, kmers, counts, alphabet_name, no_end=False, reverse=False):
        self._build_lookup(kmers, counts, alphabet_name, no_end)
        if not 1 <= self.counts.shape[1] <= kernels.GROUPS_MAX:
            raise ValueError(f"{self.counts.shape[1]} groups: a GroupCounter holds 1..{kernels.GROUPS_MAX}")
        self.reverse = bool(reverse)

    @property
    def num_groups(self):
        return int(self.counts.shape[1])

    @classmethod
    def from_dataset(cls, data, cols=None, no_end=False):
        """The columns ``cols`` (all of them by default) of a ``CountDataset`` (uploaded) or a ``DeviceCountDataset`` (gathered on its
        device): group ``g`` = column ``cols[g]``."""
        if not isinstance(data, dataloader.CountDataset):
            raise ValueError("data must be a CountDataset or a DeviceCountDataset")
        if isinstance(data, dataloader.KmerDealtDataset) or data.shard is not None:
            raise ValueError("GroupCounter.from_dataset: a sharded or k-mer-dealt table holds part of the k-mers (load it unsharded)")
        cols = list(range(data.num_ds)) if cols is None else [int(c) for c in cols]
        if not cols or any(not 0 <= c < data.num_ds for c in cols):
            raise ValueError(f"cols {cols}: the table has columns 0..{data.num_ds - 1}")
        if isinstance(data, dataloader.DeviceCountDataset):
            kmers, counts = data.kmers_dev, data.counts_dev[cols]
        else:
            device = get_var_probs._device()
            kmers = torch.from_numpy(np.ascontiguousarray(data.kmers, dtype=np.uint8)).to(device)
            counts = torch.from_numpy(np.ascontiguousarray(data.counts[cols]).view(np.int32)).to(device)
        return cls(kmers, counts.permute(1, 0, 2).contiguous(), data.alphabet, no_end=no_end)

    @classmethod
    def from_sequences(cls, seqs_by_group, lag, alphabet_name="dna", reverse=False):
        """A list of lists of sequences (str), group ``g`` = list ``g``: encoded with their group ids and counted on the device
        (``summarize.count_transitions``); the table stays where it was counted."""
        from . import summarize
        if alphabet_name == "prot" and reverse:
            raise ValueError("GroupCounter.from_sequences: the protein alphabet has no reverse complement, pass reverse=False")
        groups = [[str(s) for s in seqs] for seqs in seqs_by_group]
        if not 1 <= len(groups) <= kernels.GROUPS_MAX or any(isinstance(seqs, str) for seqs in seqs_by_group):
            raise ValueError(f"seqs_by_group: a list of 1..{kernels.GROUPS_MAX} lists of sequences, one per group")
        ids = [g for g, seqs in enumerate(groups) for _ in seqs]
        text, grp = summarize.encode_sequences([s for seqs in groups for s in seqs], ids, reverse=reverse, alphabet=alphabet_name)
        kmers, counts = summarize.count_transitions(text, grp, int(lag), len(groups), on_device=True, alphabet=alphabet_name)
        return cls(kmers, counts.permute(1, 0, 2).contiguous(), alphabet_name, reverse=reverse)


class ClassifyResult:
    """``models``: a label per model, the BEAR models (one per h) first, then the vanilla ones; ``log_marg`` float64 [n, G, M]: the
    exact log marginal of sequence ``i`` under the posterior of group ``g``; ``log_post`` float64 [n, G, M]: ``log_marg +
    log_prior[g]`` less its logsumexp over the groups; ``best`` int64 [n, M]: the group of the largest ``log_post``, the lowest
    index on a tie.  NumPy arrays."""

    def __init__(self, models, log_marg, log_post, best):
        self.models = list(models)
        self.log_marg, self.log_post, self.best = log_marg, log_post, best

    def __repr__(self):
        return f"ClassifyResult({self.log_marg.shape[0]} sequences x {self.log_marg.shape[1]} groups, models {self.models})"


def _piece_budget(device):
    """Bytes one piece of a call may take on ``device``: half of what is free, the rest stays for the rows and torch's temporaries."""
    return get_var_probs._free_memory(device) // 2


def _pieces(lengths, bytes_per_position, budget):
    """``[(lo, hi)]``: runs of whole sequences whose positions take at most ``budget`` bytes (a sequence beyond it is a piece alone)."""
    out, lo, held = [], 0, 0
    for i, n in enumerate(lengths):
        if i > lo and (held + n) * bytes_per_position > budget:
            out.append((lo, i))
            lo, held = i, 0
        held += n
    if lo < len(lengths):
        out.append((lo, len(lengths)))
    return out


def _check_call(counter, n, log_prior, own_group):
    """The refusals that need no device -> ``(log_prior float64 [G], own int32 [n] or None)``."""
    if not isinstance(counter, GroupCounter):
        raise ValueError("counter must be a GroupCounter")
    G = counter.num_groups
    log_prior = np.zeros(G) if log_prior is None else np.asarray(log_prior, dtype=np.float64)
    if log_prior.shape != (G,) or np.isnan(log_prior).any() or np.isposinf(log_prior).any():
        raise ValueError(f"log_prior: {G} log probabilities, one per group (-inf rules a group out)")
    if own_group is None:
        return log_prior, None
    own = np.asarray(own_group)
    if own.shape != (n,) or own.dtype.kind not in "iu":
        raise ValueError(f"own_group: an integer per sequence ({n}), -1 for none")
    if own.size and (own.min() < -1 or own.max() >= G):
        raise ValueError(f"own_group: groups 0..{G - 1}, or -1 for none")
    if counter.reverse:
        raise ValueError("own_group: the counter was built with reverse=True -- its table holds more of a sequence than its forward "
                         "transitions, which are all the leave-one-out marginal takes out")
    return log_prior, own.astype(np.int32)


def _resolve_models(counter, bear_path, ar_func, hs, vs):
    """What follows ``hypothesis._check_model`` once the counter is known -> ``(hs, ar_func, labels)``: a trained folder's AR function
    and fitted h (its lag and alphabet must be the table's), and a label per model, the BEAR models first."""
    if bear_path is not None:
        model_lag, model_alphabet, h_fit, ar_func, _ = get_var_probs.load_bear(bear_path)
        if model_lag != counter.lag or model_alphabet != counter.alphabet_name:
            raise ValueError(f"{bear_path}: a lag-{model_lag} model of {model_alphabet!r}, the table has lag {counter.lag} of "
                             f"{counter.alphabet_name!r}")
        hs = np.array([h_fit], dtype=np.float64)
    if hs is None:
        hs = np.zeros(0)
    return hs, ar_func, [f"bear(h={v:g})" for v in hs] + [f"van({v:g})" for v in vs]


def classify(counter, seqs, *, vans=(), bear_path=None, ar_func=None, h=None, log_prior=None, own_group=None, no_ends=False):
    """The sequences ``seqs`` (str) under every group of ``counter`` (a ``GroupCounter``) -> ``ClassifyResult``.

    Models as in ``hypothesis.two_sample``: ``bear_path`` (a trained folder's AR function and fitted h) or ``ar_func`` with ``h``
    (one value or several), and / or vanilla pseudo-counts ``vans``.  A sequence is scored as ``get_bear_probs_seqs`` scores it:
    ``lag * '[' + s + ']'`` unless ``no_ends``.  ``log_prior`` float64 [G]: the groups' log prior probabilities (uniform by default;
    a common shift cancels).  ``own_group`` int [n]: the group whose counts hold sequence ``i`` itself, -1 for none; that group's
    marginal is the leave-one-out one.  ``ValueError`` before a device is touched: the model refusals of ``hypothesis``, a prior or
    ``own_group`` of the wrong shape, ``own_group`` with a reverse-complement table; and, once scored, a sequence that is not in
    the group ``own_group`` claims (the first such sequence is named).

    The call goes through in pieces of whole sequences whose terms (positions x G x models) fit the free device memory; a
    sequence's bits depend on its content alone, so the result does not depend on the cut."""
    hs, vs = hypothesis._check_model(bear_path, ar_func, h, vans)
    seqs = [str(s) for s in seqs]
    log_prior, own = _check_call(counter, len(seqs), log_prior, own_group)
    lag, alphabet = counter.lag, counter.alphabet_name
    hs, ar_func, models = _resolve_models(counter, bear_path, ar_func, hs, vs)
    segments = seqs if no_ends else ["[" * lag + s + "]" for s in seqs]
    G, M, W, device = counter.num_groups, hs.size + vs.size, counter.width, counter.device
    with torch.cuda.device(device):
        log_marg = torch.zeros((len(seqs), G, M), dtype=torch.float64, device=device)
        per_position = (G * M + 8) * 8              # the terms, and the sort's keys, order, rows and letters
        for lo, hi in _pieces([len(s) for s in segments], per_position, _piece_budget(device)):
            _, _, text = get_var_probs._segment_rows(counter, segments[lo:hi], lag, alphabet, hs, ar_func, vs)
            if text is None:                        # no transition anywhere: zeros
                continue
            seg, rows, letters, kmer_keys, positions = text
            K = kmer_keys.numel()
            prior = get_var_probs._prior_rows(counter, ar_func, kmer_keys, K * W * (2 * G * 4 + 3 * 8) + positions * per_position,
                                              f"the rows of {K} k-mers x {G} groups x {W} letters and the terms of {positions} positions x "
                                              f"{G} groups x {M} models take", "classify fewer sequences per call")
            own_dev = None if own is None else torch.from_numpy(own[lo:hi]).to(device)
            scores, short_of = kernels.score_groups(rows, letters, seg, counter.rows_of_keys(kmer_keys), prior, hs, vs, own=own_dev)
            if own is not None and bool(short_of.any()):
                i = lo + int(torch.nonzero(short_of)[0])
                raise ValueError(f"own_group: sequence {i} ({seqs[i][:40]!r}) is not in group {int(own[i])}: that group holds one of its "
                                 "transitions fewer times than the sequence does")
            log_marg[lo:hi] = scores
        joint = log_marg + torch.from_numpy(log_prior).to(device)[None, :, None]
        log_post = joint - torch.logsumexp(joint, dim=1, keepdim=True)
        at_max = log_post == log_post.max(dim=1, keepdim=True).values
        best = torch.where(at_max, torch.arange(G, device=device)[None, :, None], G).min(dim=1).values
        return ClassifyResult(models, log_marg.cpu().numpy(), log_post.cpu().numpy(), best.cpu().numpy())


# ------------------------------------------------------------------------------------------- where in a sequence
class PositionLogProbs:
    """``models``: a label per model, the BEAR models first; ``offsets`` int64 [n + 1]: sequence ``i`` holds the rows
    ``offsets[i] .. offsets[i + 1] - 1``; ``log_prob`` float64 [P, G, M]: the posterior-predictive log-probability of the letter of
    every transition under every group and model.  NumPy arrays."""

    def __init__(self, models, offsets, log_prob):
        self.models, self.offsets, self.log_prob = list(models), offsets, log_prob

    def __repr__(self):
        return f"PositionLogProbs({self.offsets.size - 1} sequences, {self.log_prob.shape[0]} transitions x {self.log_prob.shape[1]} groups, models {self.models})"


class Segmentation:
    """``model``: the label of the model whose emissions the chain ran on; ``offsets`` int64 [n + 1] as in ``PositionLogProbs``;
    ``path`` uint8 [P]: per transition the group of the largest max-marginal (the Viterbi path wherever the best path is unique;
    255 where the chain allows no path); ``log_best`` / ``log_evidence`` float64 [n]: the best path's and all paths' log-probability
    of every sequence; ``log_post`` float64 [P, G], every transition's log posterior over the groups, or None.  NumPy arrays."""

    def __init__(self, model, offsets, path, log_best, log_evidence, log_post):
        self.model, self.offsets, self.path = model, offsets, path
        self.log_best, self.log_evidence, self.log_post = log_best, log_evidence, log_post

    def runs(self, i):
        """The stretches ``[(start, stop, group)]`` of equal group along sequence ``i``, in order: they tile ``[0, its transitions)``."""
        p = self.path[self.offsets[i]:self.offsets[i + 1]]
        if not p.size:
            return []
        cuts = np.concatenate([[0], np.flatnonzero(p[1:] != p[:-1]) + 1, [p.size]])
        return [(int(a), int(b), int(p[a])) for a, b in zip(cuts[:-1], cuts[1:])]

    def __repr__(self):
        return f"Segmentation({self.offsets.size - 1} sequences, {self.path.size} transitions, model {self.model})"


def _check_counter(counter, max_groups=None):
    if not isinstance(counter, GroupCounter):
        raise ValueError("counter must be a GroupCounter")
    if max_groups is not None and counter.num_groups > max_groups:
        raise ValueError(f"{counter.num_groups} groups: the chain of segment takes at most {max_groups} states")
    return counter.num_groups


def _emissions(counter, segments, hs, ar_func, vs, per_position):
    """The transitions of one piece -> ``(seg int64 [n + 1] on the device, emit [M, P, G])``: ``_segment_rows``, the first ``lag``
    positions of every segment -- which hold no transition -- dropped and the offsets shifted, ``_prior_rows`` and
    ``kernels.emit_groups`` on what is left.  Under the caller's device context."""
    lag, device, G, W = counter.lag, counter.device, counter.num_groups, counter.width
    M = hs.size + vs.size
    _, _, text = get_var_probs._segment_rows(counter, segments, lag, counter.alphabet_name, hs, ar_func if hs.size else None, vs)
    if text is None:
        return torch.zeros(len(segments) + 1, dtype=torch.int64, device=device), torch.zeros((M, 0, G), dtype=torch.float64, device=device)
    seg, rows, letters, kmer_keys, positions = text
    lens = seg[1:] - seg[:-1]
    keep = torch.arange(positions, dtype=torch.int64, device=device) - torch.repeat_interleave(seg[:-1], lens) >= lag
    rows, letters = rows[keep].contiguous(), letters[keep].contiguous()
    kept = torch.zeros_like(seg)
    torch.cumsum((lens - lag).clamp_(min=0), 0, out=kept[1:])
    K = kmer_keys.numel()
    prior = get_var_probs._prior_rows(counter, ar_func if hs.size else None, kmer_keys, K * W * (2 * G * 4 + 3 * 8) + positions * per_position,
                                      f"the rows of {K} k-mers x {G} groups x {W} letters and the values of {positions} positions x "
                                      f"{G} groups x {M} models take", "pass fewer sequences per call")
    return kept, kernels.emit_groups(rows, letters, counter.rows_of_keys(kmer_keys), prior, hs, vs)


def position_log_probs(counter, seqs, *, vans=(), bear_path=None, ar_func=None, h=None, no_ends=False):
    """The posterior-predictive log-probability of every transition of the sequences ``seqs`` (str) under every group of ``counter``
    (a ``GroupCounter``) and every model -> ``PositionLogProbs``.  The models of ``classify``.  A sequence is read as ``classify``
    reads it: it contributes its letters and then its stop, or with ``no_ends`` its letters behind the first ``lag``.  A row is the
    exact marginal of that single transition, ``log(a_l) - log(A)`` (include/bear_hip.h): a k-mer that no group has seen scores through
    the prior alone.  ``ValueError`` before a device is touched: the model refusals of ``hypothesis``, a counter that is no
    ``GroupCounter``.  In pieces of whole sequences that fit the free device memory; the result does not depend on the cut."""
    hs, vs = hypothesis._check_model(bear_path, ar_func, h, vans)
    seqs = [str(s) for s in seqs]
    G = _check_counter(counter)
    hs, ar_func, models = _resolve_models(counter, bear_path, ar_func, hs, vs)
    lag, M = counter.lag, hs.size + vs.size
    segments = seqs if no_ends else ["[" * lag + s + "]" for s in seqs]
    counts = np.array([max(len(s) - lag, 0) for s in segments], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    log_prob = np.zeros((int(offsets[-1]), G, M))
    per_position = (2 * G * M + 8) * 8              # the values and their transpose, and the text's keys, rows and letters
    with torch.cuda.device(counter.device):
        for lo, hi in _pieces([len(s) for s in segments], per_position, _piece_budget(counter.device)):
            _, emit = _emissions(counter, segments[lo:hi], hs, ar_func, vs, per_position)
            log_prob[offsets[lo]:offsets[hi]] = emit.permute(1, 2, 0).cpu().numpy()
    return PositionLogProbs(models, offsets, log_prob)


def _check_chain(G, switch, log_trans, log_start):
    """The chain of ``segment`` -> ``(log_trans [G, G], log_start [G])`` host float64; needs no device."""
    if (switch is None) == (log_trans is None):
        raise ValueError("give exactly one of switch (a probability of leaving a group per step) and log_trans [G, G]")
    if switch is not None:
        if log_start is not None:
            raise ValueError("switch comes with a uniform start: give log_trans to set log_start")
        if G < 2:
            raise ValueError("switch: a table of one group has no other group to switch to")
        rho = float(switch)
        if not 0.0 < rho < 1.0:
            raise ValueError(f"switch {switch}: a probability strictly between 0 and 1")
        log_trans = np.full((G, G), np.log(rho / (G - 1)))
        np.fill_diagonal(log_trans, np.log1p(-rho))
    if log_start is None:
        log_start = np.full(G, -np.log(G))
    return kernels.check_chain(log_trans, log_start, G)


def segment(counter, seqs, *, switch=None, log_trans=None, log_start=None, model=0, posterior=True, vans=(), bear_path=None, ar_func=None,
            h=None, no_ends=False):
    """Which stretch of every sequence of ``seqs`` (str) belongs to which group of ``counter`` (a ``GroupCounter`` of at most
    ``kernels.HMM_MAX_STATES`` groups) -> ``Segmentation``.  A hidden-Markov chain whose states are the groups runs over the
    transitions of a sequence (``position_log_probs``' rows under one model are its emissions).

    The chain: ``switch=rho`` -- stay with ``log(1 - rho)``, go to each other group with ``log(rho / (G - 1))``, start uniformly --
    or ``log_trans`` float64 [G, G], from-group by row, with ``log_start`` [G] (uniform by default); -inf is allowed and rows need
    not be normalised.  Exactly one of the two.  ``model``: the index of the one model the chain runs on among those the model
    arguments (``classify``'s) resolve to, the BEAR models first; only its emissions are formed.  ``posterior=False``: no
    ``log_post``.  ``ValueError`` before a device is touched: the model refusals of ``hypothesis``, a counter that is no
    ``GroupCounter`` or has more groups than the chain has states, a chain with NaN, +inf, a wrong shape or a row without a finite
    entry, ``switch`` outside (0, 1) or with a single group, a ``model`` that is none of the models.

    In pieces of whole sequences that fit the free device memory; a sequence's bits depend on its content alone, so the result
    does not depend on the cut."""
    hs, vs = hypothesis._check_model(bear_path, ar_func, h, vans)
    seqs = [str(s) for s in seqs]
    G = _check_counter(counter, kernels.HMM_MAX_STATES)
    log_trans, log_start = _check_chain(G, switch, log_trans, log_start)
    n_bear = 1 if bear_path is not None else (0 if hs is None else hs.size)
    if isinstance(model, bool) or not isinstance(model, (int, np.integer)) or not 0 <= model < n_bear + vs.size:
        raise ValueError(f"model {model!r}: an index into the {n_bear + vs.size} models, BEAR first")
    hs, ar_func, models = _resolve_models(counter, bear_path, ar_func, hs, vs)
    hs, vs = (hs[model:model + 1], vs[:0]) if model < hs.size else (hs[:0], vs[model - hs.size:model - hs.size + 1])
    lag = counter.lag
    segments = seqs if no_ends else ["[" * lag + s + "]" for s in seqs]
    counts = np.array([max(len(s) - lag, 0) for s in segments], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    P, n = int(offsets[-1]), len(seqs)
    path, log_best, log_evidence = np.zeros(P, dtype=np.uint8), np.zeros(n), np.zeros(n)
    log_post = np.zeros((P, G)) if posterior else None
    per_position = (3 * G + 8) * 8                  # the emissions, the posterior and the chain's forward values, and the text
    with torch.cuda.device(counter.device):
        for lo, hi in _pieces([len(s) for s in segments], per_position, _piece_budget(counter.device)):
            seg, emit = _emissions(counter, segments[lo:hi], hs, ar_func, vs, per_position)
            ev, best, steps, post = kernels.hmm_groups(emit[0], seg, log_trans, log_start, want_post=posterior)
            log_evidence[lo:hi], log_best[lo:hi] = ev.cpu().numpy(), best.cpu().numpy()
            path[offsets[lo]:offsets[hi]] = steps.cpu().numpy()
            if posterior:
                log_post[offsets[lo]:offsets[hi]] = post.cpu().numpy()
    return Segmentation(models[model], offsets, path, log_best, log_evidence, log_post)
