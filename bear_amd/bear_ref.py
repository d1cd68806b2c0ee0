"""Reference-based BEAR / AR models: host mirror of ``bear_model/bear_ref.py`` over the HIP kernels.

Same entry points and argument meaning as the reference: ``train`` (bear_ref.py:262-389),
``evaluation`` (:453-539), ``change_scope_params`` (:166-204).  With the stop net function
(``ar_funcs.make_ar_func_stop``, the reference's bear_stop_*.cfg configurations) a training step is one
launch of ``bear_dm_ref[_plan]_f64`` per batch shard plus one all-reduce of 4 doubles.
"""
import os

import numpy as np
import torch

from . import _train, ar_funcs as _ar_funcs, core, dist, kernels

epsilon = core.epsilon


def _counts_to_probs(ref_counts, tau, alphabet_size, dtype=torch.float64):
    """bear_ref.py:9-33."""
    norm = ref_counts / ref_counts.abs().sum(-1, keepdim=True)
    shape = torch.tensor(np.r_[np.ones(alphabet_size), 0], dtype=dtype, device=ref_counts.device)
    return (1 / alphabet_size) * shape + torch.exp(-tau) * (norm - (1 / alphabet_size) * shape)


class _FusedRefMix(torch.autograd.Function):
    """``(nw net + jukes_cantor(ref, tau)) / (nw + 1)`` (bear_ref.py:63-68) as ``bear_ref_mix_forward_f64`` /
    ``bear_ref_mix_backward_f64`` behind torch autograd: a dozen passes over [n, 5] temporaries become one launch each way."""

    @staticmethod
    def _rows(t):            # contiguous and 16-byte aligned (a slice of a larger tensor may start at an odd row)
        t = t.detach().contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()

    @staticmethod
    def forward(ctx, net_rows, ref_rows, tau_signed, net_weight_signed):
        net_rows, ref_rows = _FusedRefMix._rows(net_rows), _FusedRefMix._rows(ref_rows)
        ctx.save_for_backward(net_rows, ref_rows, tau_signed.detach(), net_weight_signed.detach())
        return kernels.ref_mix_forward(net_rows, ref_rows, tau_signed.detach(), net_weight_signed.detach())

    @staticmethod
    def backward(ctx, grad_prior):
        net_rows, ref_rows, tau_signed, net_weight_signed = ctx.saved_tensors
        grad_rows, scalars = kernels.ref_mix_backward(net_rows, ref_rows, _FusedRefMix._rows(grad_prior), tau_signed, net_weight_signed)
        return grad_rows, None, scalars[0].reshape(tau_signed.shape), scalars[1].reshape(net_weight_signed.shape)


def _make_ref_ar_func(lag, alphabet_size, make_net_func, af_kwargs, dtype=torch.float64, device=None):
    """bear_ref.py:36-69: params = [tau_signed, net_weight_signed] + net params."""
    net_weight_signed = torch.tensor(-np.log(100), dtype=dtype, device=device, requires_grad=True)
    tau_signed = torch.tensor(np.log(1 / 30), dtype=dtype, device=device, requires_grad=True)
    net_func, ar_func_params = make_net_func(lag, alphabet_size, **af_kwargs, dtype=dtype, device=device)

    def ar_func(kmer_seqs, ref_counts):
        net = net_func(kmer_seqs)
        if (alphabet_size == 4 and dtype == torch.float64 and ref_counts.is_cuda and net.is_cuda and tau_signed.is_cuda
                and net.dim() == 2 and net.shape == ref_counts.shape and ref_counts.dtype == torch.float64 and net.shape[0]):
            return _FusedRefMix.apply(net, ref_counts, tau_signed, net_weight_signed)   # one launch per direction (kernels_refmix.h)
        nw = torch.exp(net_weight_signed)
        tau = torch.exp(tau_signed)
        return (nw * net + _counts_to_probs(ref_counts, tau, alphabet_size, dtype=dtype)) / (nw + 1)
    ar_func.net_is_stop = bool(getattr(net_func, "is_stop", False))
    ar_func.net_func, ar_func.tau_signed, ar_func.net_weight_signed = net_func, tau_signed, net_weight_signed
    # the Jukes-Cantor row sums to one, so the mixture does whenever the net function's rows do (every reference AR function)
    ar_func.normalized_rows = bool(getattr(net_func, "normalized_rows", False))
    return ar_func, ([tau_signed, net_weight_signed] + ar_func_params)


def _create_params(lag, alphabet_size, make_ar_func, af_kwargs, dtype=torch.float64, device=None):
    """bear_ref.py:136-163."""
    ar_func, ar_func_params = _make_ref_ar_func(lag, alphabet_size, make_ar_func, af_kwargs, dtype, device)
    h_signed = torch.tensor(0.0, dtype=dtype, device=device, requires_grad=True)
    return [h_signed] + ar_func_params, h_signed, ar_func


def change_scope_params(lag, alphabet_size, make_ar_func, af_kwargs, params, dtype=torch.float64, device=None):
    """bear_ref.py:166-204: rebuilds (params, h_signed, ar_func) from a saved parameter list."""
    return _train.restore_params(_create_params(lag, alphabet_size, make_ar_func, af_kwargs, dtype, device), params)


def _ref_input(ref_slab, dtype=torch.float64):
    """bear_ref.py:332-337: ``(counts[:, ds_loc_ref] + epsilon) * not_stop``."""
    r = _train.counts_f64(ref_slab).to(dtype) + epsilon
    r[:, -1] = 0
    return r


def _planned_step(res, theta, train_ar):
    """``make(k)`` of the stop net function on 5-wide rows (``_train.reducers``): the mode-R kernel over a plan."""
    def make(k):
        e = res.load(k)
        if e["rows"] == 0:
            return _train.zero_reduce
        # built here, before any capture (plan creation allocates and synchronises); the reference column is resident too, so the
        # plan folds the contexts without reference counts into a histogram and a step streams only the others' items
        plan = res.plan(k, "train", 4, ref_column="ref")
        return _train.StepFns(
            lambda packed: kernels.ref_train_reduce(plan, e["ref"], theta, packed, train_ar=train_ar),
            lambda packed, m, v, t, lr, scale, loss_buf: kernels.ref_train_step(plan, e["ref"], theta, m, v, t, lr, scale, packed, loss_buf,
                                                                                train_ar=train_ar))
    return make


def _wide_step(res, theta, train_ar):
    """``make(k)`` of the stop net function on rows of 21: dm_ref_wide_kernel on the count rows, no plan."""
    def make(k):
        e = res.load(k)
        if e["rows"] == 0:
            return _train.zero_reduce
        return _train.StepFns(
            lambda packed: kernels.ref_train_reduce_wide(e["train"], e["ref"], theta, packed, train_ar=train_ar),
            lambda packed, m, v, t, lr, scale, loss_buf: kernels.ref_train_step_wide(e["train"], e["ref"], theta, m, v, t, lr, scale,
                                                                                     packed, loss_buf, train_ar=train_ar))
    return make


def train(data, num_kmers, epochs, ds_loc, ds_loc_ref, alphabet, lag, make_ar_func, af_kwargs,
          learning_rate, optimizer_name, train_ar, acc_steps=1,
          params_restart=None, writer=None, loss_save=None, dtype=torch.float64):
    """bear_ref.train (bear_ref.py:262-389).  ``data`` is the (repeated) CountDataset of
    ``bear_amd.dataloader``; rows of every batch are sharded over the ranks of an initialised
    ``torch.distributed`` group (one process per GPU).  Returns ``(params, h_signed, ar_func)``."""
    dtype = _train.compute_dtype(dtype)              # float32 configs run in float64 too (the reference recommends float64)
    device = _train.require_device()
    alphabet_size = len(core.alphabets_tf[alphabet]) - 1
    if params_restart is None:
        params, h_signed, ar_func = _create_params(lag, alphabet_size, make_ar_func, af_kwargs, dtype, device)
    else:
        params, h_signed, ar_func = change_scope_params(lag, alphabet_size, make_ar_func, af_kwargs, params_restart, dtype, device)
    dist.broadcast_params(params)                    # mirrored variables: every rank starts from rank 0's values (bear_ref.py:310-321)
    width = _train.row_width(data)
    wide = width != 5
    if not ar_func.net_is_stop or (wide and (width not in kernels.WIDE_WIDTHS or os.environ.get("BEAR_AMD_UNFUSED_MIX"))):
        # (a net function with parameters; or, BEAR_AMD_UNFUSED_MIX=1, a protein table the former way: the mixing as torch ops around
        # the width-generic mode-N kernel -- tests and scripts/prot_ref_time.py compare the two)
        return _train_general(data, num_kmers, params, h_signed, ar_func, learning_rate, optimizer_name, train_ar, acc_steps, writer,
                              loss_save, ds_loc, ds_loc_ref, device)
    # stop net function: theta = (h_signed, tau_signed, net_weight_signed) lives on the device for the whole run; one step is
    # constants-from-theta -> mode-R kernel -> finalize [-> all-reduce of 4 doubles] -> Adam, no host round trip
    res = _train.ResidentBatches(data, {"train": ds_loc, "ref": ds_loc_ref}, device, drop_empty="train",
                                 prebuild=[("train", 4, "ref")])       # plans cut while the next batch is still crossing PCIe
    theta = _train.pack_theta(params[:3], device)
    make = _wide_step(res, theta, train_ar) if wide else _planned_step(res, theta, train_ar)
    losses = _train.run_device_steps(_train.reducers(res, make), _train.loss_scales(res, num_kmers), theta, data.repeats, learning_rate,
                                     optimizer_name, train_ar, acc_steps, device, graph_ok=not res.streaming)
    res.close()
    _train.unpack_theta(theta, params[:3])
    _train.log_losses(losses, writer, loss_save, acc_steps)
    return params, h_signed, ar_func


def _train_general(data, num_kmers, params, h_signed, ar_func, learning_rate, optimizer_name, train_ar, acc_steps, writer, loss_save,
                   ds_loc, ds_loc_ref, device):
    """bear_ref.train with a parametrised net function (linear, cnn; bear_ref.py:63-68).  Per batch: the net function's rows
    (``bear_linear_forward_f64`` / ``bear_cnn_forward_f64`` behind autograd), then ONE launch of ``bear_dm_refmix_plan_grad_f64``
    -- the mixing ``(nw net + jukes_cantor(ref, tau)) / (nw + 1)``, sum LL, d/dh, d/dtau, d/dnet_weight and d/d(net rows) -- and
    the net function's backward launch.  Net rows that are not asserted normalised (a plugin without ``normalized_rows``) take
    three launches instead: ``bear_ref_mix_forward_f64``, the planned kernel with gradient rows, ``bear_ref_mix_backward_f64``
    through autograd -- the same loop as bear_net.train with two more parameters.  A protein table (rows of 21) takes
    ``bear_dm_refmix_wide_grad_f64`` in the place of the planned launch, on the count rows of both columns; with
    BEAR_AMD_UNFUSED_MIX=1 it mixes in torch ops around ``bear_dm_prior_wide_f64`` (with the stop net function too)."""
    # a fused net function (linear rows / cnn kernels) shares work between neighbouring contexts: batches are kept in k-mer order
    # (the sums do not depend on the order; cnn forward + backward 70 instead of 137 ms per 1e8 contexts, linear backward 1.45 / 2.0);
    # the 4-letter kernels only: the rows of 21 (kernels_linrows_wide.h) share nothing between neighbours, and the sort packs 3 bits
    width = _train.row_width(data)
    res = _train.ResidentBatches(data, {"train": ds_loc, "ref": ds_loc_ref}, device, want_codes=True, drop_empty="train",
                                 kmer_order=bool(getattr(getattr(ar_func, "net_func", None), "fused", False)) and width == 5,
                                 prebuild=[("train", 5, None)], per_row_extra=24 * width)

    def with_ref_in(e):
        if "ref_in" not in e:
            e["ref_in"] = _ref_input(e["ref"])
        return e

    def prior_fn(e):                 # (contexts without training counts need no prior row)
        return _train.rows_on_live(with_ref_in(e), ar_func, columns=("codes", "ref_in")).contiguous()
    # normalised net rows, the reference's own mixing parameters: the mixing runs inside the DM kernel
    # (bear_dm_refmix_plan_grad_f64: one launch instead of mix-forward, gradient rows, mix-backward); BEAR_AMD_UNFUSED_MIX=1 keeps
    # the three launches (tests compare the two)
    # Rows of 21: the same in bear_dm_refmix_wide_grad_f64, from the reference COUNTS (no fp64 reference rows exist) and for any
    # non-negative net rows (the kernel forms their sums itself: no normalized_rows promise needed)
    ref_mix = None
    own_mix = (getattr(ar_func, "net_func", None) is not None and params[1] is ar_func.tau_signed and params[2] is ar_func.net_weight_signed
               and not os.environ.get("BEAR_AMD_UNFUSED_MIX"))
    if own_mix and (ar_func.normalized_rows if width == 5 else width in kernels.WIDE_WIDTHS):
        if width == 5:               # (the live contexts' reference rows are gathered next to their codes, as for prior_fn)
            net_fn = lambda e: _train.rows_on_live(with_ref_in(e), lambda codes, ref_in: ar_func.net_func(codes), columns=("codes", "ref_in"))
        else:
            net_fn = lambda e: _train.rows_on_live(e, ar_func.net_func)
        ref_mix = (net_fn, (lambda e: e["ref_in"]) if width == 5 else (lambda e: e["ref"]), params[1], params[2])
    losses = _train.run_autograd_steps(res, prior_fn, params, h_signed, num_kmers, data.repeats, learning_rate, optimizer_name, train_ar,
                                       acc_steps, ar_func.normalized_rows, device, ref_mix=ref_mix)
    res.close()
    _ar_funcs.release_ar_func_cache(getattr(ar_func, "net_func", ar_func))
    _train.log_losses(losses, writer, loss_save, acc_steps)
    return params, h_signed, ar_func


def evaluation(data, ds_loc_train, ds_loc_test, ds_loc_ref, alphabet, h, ar_func, van_reg, dtype=torch.float64,
               seed=0):
    """bear_ref.evaluation (bear_ref.py:453-539) -> (ll_ear, ll_arm, ll_van, perp_ear, perp_arm, perp_van,
    acc_ear, acc_arm, acc_van).  ``ds_loc_train = -1``: no conditioning on training counts.  The training
    column is used for conditioning (the reference reads the reference column there by mistake,
    bear_ref.py:397 vs bear_net.py:327)."""
    dtype = _train.compute_dtype(dtype)
    device = _train.require_device()
    cols = {"test": ds_loc_test, "ref": ds_loc_ref, **({"train": ds_loc_train} if ds_loc_train >= 0 else {})}
    hv = float(torch.as_tensor(h).item()) if np.ndim(torch.as_tensor(h).detach().cpu().numpy()) == 0 else torch.as_tensor(h).detach().cpu().numpy()

    def prior_rows(e, suffix):
        if "ref_in" not in e:
            e["ref_in"] = _ref_input(e["ref"], dtype)
        _train.live_rows(e, "ref_in", by="test")         # (gathers the live contexts' reference rows next to their codes)
        return ar_func(e["codes" + suffix], e["ref_in" + suffix])
    total = _train.evaluate_resident(data, cols, hv, van_reg, seed, dtype, device, prior_rows, getattr(ar_func, "net_func", ar_func))
    return _train.reduce_evaluation(total, device, np.ndim(hv) == 0)
