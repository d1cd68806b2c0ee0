"""BEAR / AR models with a parametric AR function: host mirror of ``bear_model/bear_net.py``.

``train`` (bear_net.py:200-321), ``evaluation`` (:387-463), ``h_scan`` (:465-531),
``change_scope_params`` (:103-143) with the reference's signatures.  Per batch shard and step the
AR rows come from the plugin (``ar_funcs``, PyTorch-ROCm ops with autograd), and the DM / multinomial
log-likelihood, its gradient w.r.t. ``h_signed`` and w.r.t. the AR rows come from one launch of
``bear_dm_prior_f64``; the row gradient is fed back through ``ar_func`` by ``Tensor.backward``.  The reference's linear and
convolutional AR functions take fused steps instead, at either alphabet width (``step_form``).
"""
import os

import numpy as np
import torch

from . import _train, ar_funcs, core, dist, kernels

epsilon = core.epsilon


def _create_params(lag, alphabet_size, make_ar_func, af_kwargs, dtype=torch.float64, device=None):
    """bear_net.py:73-100."""
    ar_func, ar_func_params = make_ar_func(lag, alphabet_size, **af_kwargs, dtype=dtype, device=device)
    h_signed = torch.tensor(0.0, dtype=dtype, device=device, requires_grad=True)
    return [h_signed] + ar_func_params, h_signed, ar_func


def change_scope_params(lag, alphabet_size, make_ar_func, af_kwargs, params, dtype=torch.float64, device=None):
    """bear_net.py:103-143."""
    return _train.restore_params(_create_params(lag, alphabet_size, make_ar_func, af_kwargs, dtype, device), params)


def linear_wide_step_selected(alphabet_size, lag, own_mat, width):
    """Whether ``train`` runs the protein alphabet's linear step as one launch per optimizer step (``bear_net_linear_train_step_wide_f64``,
    theta device-resident): the 20-letter alphabet on a 21-wide table, a lag whose mat fits the kernel's LDS, and an AR function
    whose only parameter is the linear mat itself (``own_mat``: ``ar_func.linear_mat is ar_params[0]``).
    BEAR_AMD_UNFUSED_LINEAR_WIDE=1 keeps the three row kernels under autograd (tests and scripts/prot_linear_step_time.py compare)."""
    unfused = os.environ.get("BEAR_AMD_UNFUSED_LINEAR_WIDE", "")
    return bool(alphabet_size == 20 and width == kernels.LINEAR_WIDE_WIDTH and 1 <= lag <= kernels.LINEAR_WIDE_MAX_LAG and own_mat
                and not (unfused and unfused != "0"))


def cnn_wide_step_selected(ar_func, ar_params, alphabet_size, lag, width):
    """Whether ``train`` runs the protein alphabet's convolutional step as two launches per optimizer step
    (``bear_net_cnn_train_step_wide_f64``, theta device-resident): the 20-letter alphabet on a 21-wide table, the fused AR function
    of ``make_ar_func_cnn`` whose eight parameters ARE the kernels' (identity), and a shape the kernels take (``kernels.cnn_supported``:
    30 filters, layer-1 width 16, 1 <= filter width <= lag <= 16).  Every shape timed is at least as fast as the three row kernels
    under autograd (profiles/prot_cnn_step_time.jsonl).  BEAR_AMD_UNFUSED_CNN_WIDE=1 keeps those (tests and
    scripts/prot_cnn_step_time.py compare)."""
    unfused = os.environ.get("BEAR_AMD_UNFUSED_CNN_WIDE", "")
    own = getattr(ar_func, "cnn_params", None)
    return bool(alphabet_size == 20 and width == kernels.LINEAR_WIDE_WIDTH and getattr(ar_func, "fused", False)
                and len(ar_params) == 8 and own is not None and len(own) == 8 and all(a is b for a, b in zip(own, ar_params))
                and kernels.cnn_supported(lag, 20, getattr(ar_func, "cnn_filter_width", 0), kernels.CNN_NUM_FILTERS, kernels.CNN_LAYER1_WIDTH)
                and not (unfused and unfused != "0"))


def step_form(ar_func, ar_params, alphabet_size, lag, width):
    """How ``train`` runs an optimizer step with this AR function, and the ``ResidentBatches`` keyword arguments that go with it:
    ``"linear"`` / ``"cnn"`` (a 4-letter alphabet's fused heads: forward, ELBO and all gradients in one launch per batch),
    ``"linear_wide"`` / ``"cnn_wide"`` (the protein alphabet's steps: ``linear_wide_step_selected``, ``cnn_wide_step_selected``), or
    None (torch ops under autograd).
    A fused form needs the AR function's parameters to BE the kernels' (identity, not equality)."""
    mat = getattr(ar_func, "linear_mat", None)
    # Fused heads: the sums of a step do not depend on the order of a batch's rows, so every batch is kept sorted by k-mer (first
    # letter most significant) -- consecutive contexts share all but their last letters: the fused linear kernel adds whole waves /
    # quads of them to d/d mat at once instead of one LDS atomic per context, letter and position (kernels_linear.h), the
    # convolutional kernels evaluate a window that all contexts of a wave share once (kernels_cnn.h).  The plans are cut as the
    # batches land, while the next batch is still being uploaded.  per_row_extra: plan + paired lists / prefix levels and buffers
    if mat is not None and alphabet_size == 4 and lag <= kernels.LINEAR_MAX_LAG and mat is ar_params[0]:
        return "linear", dict(kmer_order=True, prebuild=[("train", 5, None)], per_row_extra=8 + 4)
    if (getattr(ar_func, "fused", False) and alphabet_size == 4 and len(ar_params) == 8
            and all(a is b for a, b in zip(getattr(ar_func, "cnn_params", []), ar_params))):
        return "cnn", dict(kmer_order=True, prebuild=[("train", 5, None)], per_row_extra=8 + 208 + 64)
    # ... and on the protein alphabet: the linear head on int8 codes in table order (no plan, no k-mer sort: kernels_linear_wide.h)
    if linear_wide_step_selected(alphabet_size, lag, mat is not None and len(ar_params) == 1 and mat is ar_params[0], width):
        return "linear_wide", dict(kmer_order=False, prebuild=[("train", _train.ROWS_IF_DENSE, None)], per_row_extra=0)
    # ... the convolutional head likewise, in two launches (kernels_cnn_wide.h); per_row_extra: the dz and t1 rows of the step's one
    # buffer pair, 8 * (21 + 16) B per context of the largest batch
    if cnn_wide_step_selected(ar_func, ar_params, alphabet_size, lag, width):
        return "cnn_wide", dict(kmer_order=False, prebuild=[("train", _train.ROWS_IF_DENSE, None)],
                                per_row_extra=8 * (kernels.LINEAR_WIDE_WIDTH + kernels.CNN_LAYER1_WIDTH))
    return None, dict(kmer_order=False, prebuild=[("train", _train.ROWS_IF_DENSE, None)], per_row_extra=16 * (alphabet_size + 1))


def _kmer_pack(e, lag, linear):
    """The batch's k-mers as the fused kernels read them (kept with the batch): packed letters, or -- the linear head -- table-row words."""
    if "pack" not in e:
        q = kernels.pack_kmers(e["codes"].contiguous())
        e["pack"] = kernels.linear_index(q, lag) if linear else q
    return e["pack"]


def _linear_step(res, theta, lag, train_ar, device):
    """``make(k)`` of the fused linear form (``_train.reducers``)."""
    def make(k):
        e = res.load(k)
        plan = res.plan(k, "train", 5) if e["rows"] else None     # built here, before any capture (plan creation allocates and synchronises)
        if _train.deterministic_agreed(device):
            # BEAR_AMD_DETERMINISTIC: the fixed-point scale of the linear step's gradient tables follows from the counts of the
            # WHOLE batch -- every rank's piece -- so that d/d mat does not depend on the number of ranks (include/bear_hip.h);
            # a rank whose piece of the batch is empty takes part in the two all-reduces with zeros
            own = plan.count_total()[0] if plan is not None else [0.0, 0.0, 0.0]
            tot, cmax = torch.tensor(own[:2], dtype=torch.float64, device=device), torch.tensor(own[2:], dtype=torch.float64, device=device)
            dist.allreduce_sum_(tot)
            dist.allreduce_max_(cmax)
            if plan is not None:
                plan.set_count_bound(tot.tolist() + cmax.tolist())
        if plan is None:
            return _train.zero_reduce
        pack = _kmer_pack(e, lag, linear=True)
        if pack.data_ptr() % 16 == 0:
            # neighbours of the sorted batch that share all letters but the last three go through the step two at a time
            # (kernels_linear.h, paired lists); declined by the library for tables too sparse to gain from it
            plan.pair_contexts(pack, lag)
        return _train.StepFns(
            lambda packed: kernels.net_linear_train_reduce(plan, pack, lag, theta, packed, train_ar=train_ar),
            lambda packed, m, v, t, lr, scale, loss_buf: kernels.net_linear_train_step(plan, pack, lag, theta, m, v, t, packed, lr, scale,
                                                                                       loss_buf, train_ar=train_ar))
    return make


def _cnn_step(res, theta, lag, fw, train_ar, device):
    """``make(k)`` of the fused convolutional form: a reduce per batch (the update is ``run_device_steps``' own launch)."""
    cnn_ws = kernels.default_workspace(device)     # the workspace the plans below are created on: the step's reservation lives there
    bufs = kernels.cnn_step_buffers(max(max(e["rows"] for e in res.batches), 1), lag, fw, device, ws=cnn_ws)   # one set, largest batch

    def make(k):
        e = res.load(k)
        plan = res.plan(k, "train", 5) if e["rows"] else None     # (before any capture, as above)
        _train.deterministic_agreed(device)        # (the ranks' one-time agreement on the mode: its collectives come here in every fused form)
        if plan is None:
            return _train.zero_reduce
        pack = _kmer_pack(e, lag, linear=False)
        if pack.data_ptr() % 16 == 0:
            # a position of the sorted batch once per distinct prefix (kernels_cnn.h, prefix levels); none attached when the
            # prefixes of the table do not repeat
            plan.attach_cnn_levels(pack, lag, fw)
        views = tuple(b[:e["rows"]] for b in bufs)
        return lambda packed: kernels.net_cnn_train_reduce(plan, pack, lag, fw, theta, views, packed, train_ar=train_ar)
    return make


def _linear_wide_step(res, theta, lag, train_ar):
    """``make(k)`` of the protein alphabet's linear form: count rows and codes as they are, 16-byte aligned."""
    def make(k):
        e = res.load(k)
        if not e["rows"]:
            return _train.zero_reduce
        counts, codes = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (e["train"].contiguous(), e["codes"].contiguous()))
        return _train.StepFns(
            lambda packed: kernels.net_linear_train_reduce_wide(counts, codes, lag, theta, packed, train_ar=train_ar),
            lambda packed, m, v, t, lr, scale, loss_buf: kernels.net_linear_train_step_wide(counts, codes, lag, theta, m, v, t, packed, lr,
                                                                                            scale, loss_buf, train_ar=train_ar))
    return make


def _cnn_wide_step(res, theta, lag, fw, train_ar, device):
    """``make(k)`` of the protein alphabet's convolutional form: count rows and codes as they are, 16-byte aligned, and ONE pair of
    dz / t1 buffers sized for the largest batch (steps on one stream run one after the other)."""
    bufs = kernels.cnn_step_buffers_wide(max([e["rows"] for e in res.batches] + [1]), device)

    def make(k):
        e = res.load(k)
        if not e["rows"]:
            return _train.zero_reduce
        counts, codes = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (e["train"].contiguous(), e["codes"].contiguous()))
        return _train.StepFns(
            lambda packed: kernels.net_cnn_train_reduce_wide(counts, codes, lag, fw, theta, bufs, packed, train_ar=train_ar),
            lambda packed, m, v, t, lr, scale, loss_buf: kernels.net_cnn_train_step_wide(counts, codes, lag, fw, theta, m, v, t, bufs, packed,
                                                                                         lr, scale, loss_buf, train_ar=train_ar))
    return make


def train(data, num_kmers, epochs, ds_loc, alphabet, lag, make_ar_func, af_kwargs,
          learning_rate, optimizer_name, train_ar, acc_steps=1,
          params_restart=None, writer=None, loss_save=None, dtype=torch.float64):
    """bear_net.train (bear_net.py:200-321); returns ``(params, h_signed, ar_func)``."""
    dtype = _train.compute_dtype(dtype)
    device = _train.require_device()
    alphabet_size = len(core.alphabets_tf[alphabet]) - 1
    if params_restart is None:
        params, h_signed, ar_func = _create_params(lag, alphabet_size, make_ar_func, af_kwargs, dtype, device)
    else:
        params, h_signed, ar_func = change_scope_params(lag, alphabet_size, make_ar_func, af_kwargs, params_restart, dtype, device)
    dist.broadcast_params(params)                    # mirrored variables: every rank starts from rank 0's values (bear_net.py:246-256)
    form, res_kw = step_form(ar_func, params[1:], alphabet_size, lag, _train.row_width(data))
    res = _train.ResidentBatches(data, {"train": ds_loc}, device, want_codes=True, drop_empty="train", **res_kw)
    if form is None:
        normalized = bool(getattr(ar_func, "normalized_rows", False))   # every reference AR function ends in a softmax
        # (contexts without training counts need no prior row; a parameter-free AR function may return one row for all contexts)
        losses = _train.run_autograd_steps(res, lambda e: _train.rows_on_live(e, ar_func, width=alphabet_size + 1), params, h_signed,
                                           num_kmers, data.repeats, learning_rate, optimizer_name, train_ar, acc_steps, normalized, device)
    else:
        # theta = {h_signed, flattened AR parameters} lives on the device for the whole run: one step is constants-from-theta ->
        # fused kernels [-> all-reduce of the packed vector] -> Adam, no host round trip (_train.run_device_steps)
        theta = _train.pack_theta(params, device)
        graph_ok = not res.streaming
        if form == "linear":
            make = _linear_step(res, theta, lag, train_ar, device)
        elif form == "cnn":
            make = _cnn_step(res, theta, lag, ar_func.cnn_filter_width, train_ar, device)
        else:
            make = (_linear_wide_step(res, theta, lag, train_ar) if form == "linear_wide"
                    else _cnn_wide_step(res, theta, lag, ar_func.cnn_filter_width, train_ar, device))
            # the fused step pins no autograd intermediates in a graph's pool: no row cap of its own, but one that is set is honoured
            # (the tests force the eager loop of a protein run with BEAR_AMD_GRAPH_MAX_ROWS=0)
            cap = os.environ.get("BEAR_AMD_GRAPH_MAX_ROWS")
            graph_ok = graph_ok and (cap is None or max([e["global_rows"] for e in res.batches] + [0]) <= int(cap))
        losses = _train.run_device_steps(_train.reducers(res, make), _train.loss_scales(res, num_kmers), theta, data.repeats, learning_rate,
                                         optimizer_name, train_ar, acc_steps, device, graph_ok=graph_ok)
        _train.unpack_theta(theta, params)
    res.close()
    ar_funcs.release_ar_func_cache(ar_func)
    _train.log_losses(losses, writer, loss_save, acc_steps)
    return params, h_signed, ar_func


def _eval(data, ds_loc_train, ds_loc_test, alphabet, h, ar_func, van_reg, dtype, seed):
    dtype = _train.compute_dtype(dtype)
    device = _train.require_device()
    cols = {"test": ds_loc_test, **({"train": ds_loc_train} if ds_loc_train >= 0 else {})}
    total = _train.evaluate_resident(data, cols, h, van_reg, seed, dtype, device, lambda e, suffix: ar_func(e["codes" + suffix]), ar_func)
    return total, device


def evaluation(data, ds_loc_train, ds_loc_test, alphabet, h, ar_func, van_reg, dtype=torch.float64, seed=0):
    """bear_net.evaluation (bear_net.py:387-463) -> the reference's 9-tuple."""
    hv = float(torch.as_tensor(h).detach().cpu().item())
    total, device = _eval(data, ds_loc_train, ds_loc_test, alphabet, hv, ar_func, van_reg, dtype, seed)
    return _train.reduce_evaluation(total, device, True)


def h_scan(data, ds_loc_train, ds_loc_test, alphabet, h, ar_func, dtype=torch.float64, seed=0):
    """bear_net.h_scan (bear_net.py:465-531): BEAR log-likelihood, perplexity and accuracy for a vector of h."""
    hs = torch.as_tensor(h).detach().cpu().numpy().reshape(-1)
    total, device = _eval(data, ds_loc_train, ds_loc_test, alphabet, hs, ar_func, np.ones(1), dtype, seed)
    r = _train.reduce_evaluation(total, device, False)
    return r[0], r[3], r[6]
